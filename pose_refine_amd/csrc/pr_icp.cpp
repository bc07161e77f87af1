// pr_icp.cpp -- the batched ICP driver (cuda_icp/icp.cu:156-217 for many clouds): device-solve loop, host-solve pipeline, graph cache
#include "pr_runtime.h"
// what a polling loop does between two looks (HostRun::wait_flag): the pause instruction of x86, yield on aarch64, elsewhere a compiler barrier
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#define cpu_relax() _mm_pause()
#elif defined(__aarch64__)
#define cpu_relax() __asm__ __volatile__("yield" ::: "memory")
#else
#define cpu_relax() __asm__ __volatile__("" ::: "memory")
#endif

namespace prr {

hipError_t launch_pass(const prk::IcpBatch &b, const SceneSel &sc, uint32_t P, hipStream_t st, hipEvent_t *nn_marks)
{
    if (!st) st = g->stream;
    if (sc.kind == PR_SCENE_NN) {
        if (sc.nn_split && b.nn_prev) {                            // search (applies the pending update, leaves the winners in nn_prev) ...
            hipError_t e = prk::launch_nn_search(b, sc.nn, P, sc.nn_max_points, (uint32_t)std::max(1, opt.nn_run), st, nn_marks);
            if (e != hipSuccess) return e;
            prk::IcpBatch bb = b;                                   // ... then the canonical-order pass over the winners
            bb.pre_transformed = 1;
            const prk::SceneNNWinners w{ sc.nn.max_dist_diff, sc.nn.pts, sc.nn.normal, b.nn_prev };
            return prk::launch_icp_pass_nn_winners(bb, w, P, st);
        }
        prk::NNPassRan ran{};
        const hipError_t e = prk::launch_icp_pass_nn(b, sc.nn, P, st, &ran);
        g_nn_lds_nodes.store(ran.lds_nodes); g_nn_stack_depth.store(ran.stack_depth); g_nn_pass_launches.fetch_add(1);
        return e;
    }
    if (sc.kind == PR_SCENE_GRID) return prk::launch_icp_pass_grid(b, sc.grid, P, st);
    if (sc.packed) return prk::launch_icp_pass_proj_packed(b, sc.pk, P, st);
    return prk::launch_icp_pass_proj_aos(b, sc.aos, P, st);
}

// Streams are created only when they are first needed: the runtime multiplexes all streams of a process onto a handful of
// hardware queues (4 by default) in creation order, and two streams that share a queue serialise -- with every possible
// stream created up front, a slot's render stream ended up behind the other slot's 21 queued passes.
int ensure_stream(hipStream_t &st, hipEvent_t *ev)
{
    if (!st) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (ev && !*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return PR_OK;
}

// The host's part of an iteration for one hypothesis whose 29 sums Ab have arrived (icp.cu:178-212): scores, convergence test, 6x6 solve,
// accumulation of the transform into r.T.  Returns whether the hypothesis goes on; then E holds the update.  (The host-solve loop and
// pr_debug_pose_iteration both run it.)
bool pose_iteration_host(const float *Ab, uint32_t n, pr_result &r, const pr_criteria &crit, uint32_t it, float E[16])
{
    const float prev_fit = r.fitness, prev_rmse = r.inlier_rmse;
    const float cnt = Ab[28], err = Ab[27];
    if (cnt == 0) return false;                                                       // icp.cu:183
    r.fitness = cnt / (float)n;                                                       // icp.cu:185
    r.inlier_rmse = std::sqrt(err / cnt);                                             // icp.cu:186
    if (it == (uint32_t)crit.max_iteration) return false;                             // icp.cu:189
    if (std::fabs(r.fitness - prev_fit) < crit.relative_fitness &&
        std::fabs(r.inlier_rmse - prev_rmse) < crit.relative_rmse) return false;     // icp.cu:191-194
    float A[36], bb[6];
    for (int k = 0; k < 6; ++k) bb[k] = Ab[21 + k];
    int sh = 0;
    for (int y = 0; y < 6; ++y) for (int x = y; x < 6; ++x) { A[x + y * 6] = Ab[sh]; A[y + x * 6] = Ab[sh]; ++sh; }   // icp.cu:196-205
    prh::solve_666(A, bb, E);
    prh::mat4_mul(E, r.T, r.T);                                                       // icp.cu:212
    return true;
}

// ---- audit recorder (pr_debug_trace_sums) ----------------------------------------------------------
thread_local SumsTraceState tl_sums_trace;
int sums_trace_admits(const char *fn, uint32_t P, const pr_criteria &crit)
{
    const SumsTrace &t = tl_sums_trace.active;
    if (!t.rows) return PR_OK;
    if (opt.solve_mode == PR_SOLVE_DEVICE) { set_error("%s: pr_debug_trace_sums records the host-solve loop; the solve is on the device (option solve)", fn); return PR_ERR_INVALID; }
    if (P != t.n_hyp) { set_error("%s: pr_debug_trace_sums was armed for %u hypotheses, the batch has %u", fn, t.n_hyp, P); return PR_ERR_INVALID; }
    if (crit.max_iteration < 0 || (uint64_t)crit.max_iteration + 1 > t.n_passes) { set_error("%s: pr_debug_trace_sums was armed for %u passes, max_iteration %d needs %lld", fn, t.n_passes, crit.max_iteration, (long long)crit.max_iteration + 1); return PR_ERR_INVALID; }
    return PR_OK;
}

// ---- the batched ICP driver -----------------------------------------------------------------------
// What icp_drive sets up once for either driver: the batch as the passes take it, the host copies of the per-hypothesis records and results.
struct IcpRun {
    prk::IcpBatch b{}; SceneSel sc; pr_criteria crit{}; uint32_t P = 0; const uint32_t *count_h = nullptr; pr_result *results_host = nullptr, *results_dev = nullptr;
    prk::PoseMeta *h_meta = nullptr; float *h_sums = nullptr; pr_result *res = nullptr;      // pinned: g->h_meta, g->h_sums, g->h_results
    SumsTrace trace;
};

// the context's graph of `key`: looked up, or -- the least recently used of 8 evicted -- captured from enqueue() on the context's stream and instantiated; stamped
template <class Enqueue>
int cached_graph(const GraphKey &key, Enqueue &&enqueue, CachedGraph *&hit)
{
    hit = nullptr;
    for (auto &c : g->graphs) if (c.exec && c.key == key) { hit = &c; break; }
    if (!hit) {
        if (g->graphs.size() >= 8) {                         // evict the least recently used entry
            size_t lru = 0;
            for (size_t i = 1; i < g->graphs.size(); ++i) if (g->graphs[i].stamp < g->graphs[lru].stamp) lru = i;
            destroy_graph(g->graphs[lru]);
            g->graphs.erase(g->graphs.begin() + lru);
        }
        CachedGraph c; c.key = key;
        HIP_TRY(hipStreamSynchronize(g->stream));
        HIP_TRY(hipStreamBeginCapture(g->stream, hipStreamCaptureModeThreadLocal));
        const uint64_t nn_before = g_nn_pass_launches.load();
        int rc = enqueue();
        if (g_nn_pass_launches.load() != nn_before) { c.nn_pass = true; c.nn_lds_nodes = g_nn_lds_nodes.load(); c.nn_stack_depth = g_nn_stack_depth.load(); }
        hipError_t ce = hipStreamEndCapture(g->stream, &c.graph);
        if (rc != PR_OK || ce != hipSuccess) { destroy_graph(c); if (rc == PR_OK) { set_error("hipStreamEndCapture failed: %s", hipGetErrorString(ce)); rc = PR_ERR_HIP; } return rc; }
        HIP_TRY(hipGraphInstantiate(&c.exec, c.graph, nullptr, nullptr, 0));
        g->graphs.push_back(std::move(c));
        hit = &g->graphs.back();
    }
    hit->stamp = ++g->graph_clock;
    return PR_OK;
}
int drive_device(IcpRun &r)
{
    const uint32_t P = r.P;
    const pr_criteria crit = r.crit;
    PR_TRY(g->dstate.ensure(sizeof(prk::DevIcpState) * P));
    PR_TRY(g->h_dstate.ensure(sizeof(prk::DevIcpState) * P));
    prk::DevIcpState *init = g->h_dstate.as<prk::DevIcpState>();
    for (uint32_t i = 0; i < P; ++i) { identity16(init[i].T); init[i].fitness = 0; init[i].rmse = 0; init[i].done = (r.h_meta[i].state == prk::kSkip); init[i].passes = 0; }
    pr_result *dres = r.results_dev;
    if (!dres) { PR_TRY(g->dresults.ensure(sizeof(pr_result) * P)); dres = g->dresults.as<pr_result>(); }
    const bool fused = opt.fused_solve != 0;
    if (fused) PR_TRY(g->arrive.ensure(sizeof(uint32_t) * P));

    // profile==2: every sample_period-th call is a timed call -- it runs synchronously, as one pose group, with the other slot
    // drained, and times every correspondence launch of its loop
    const uint64_t tick = g->sample_clock++;
    const bool sample_call = (opt.profile == 2) && (tick % (uint64_t)std::max(1, opt.sample_period) == 0);
    // Pose groups: the batch is split over up to four streams so that one group's serial solve tail (and the ragged end
    // of its pass) overlaps another group's pass -- while the (latency-bound, one wavefront per pose) finalize+solve of one group
    // runs, the correspondence pass of the other group keeps the chip busy.  Timed launches (profile 1, the sampled call of
    // profile 2) run as a single group so that the measured kernel has the chip to itself.
    const bool timed_call = (opt.profile == 1 || opt.profile == 3) || sample_call;   // (profile 3 only keeps SUBMITTED batches asynchronous: whatever runs here is a synchronous timed call)
    const bool may_exit_early = (crit.relative_fitness > 0.0f && crit.relative_rmse > 0.0f);
    const uint32_t n_groups = pose_group_count(r.sc.kind, P, timed_call);
    const Lanes lanes{ g->stream, g->side, g->ev_fork, g->ev_join };
    // the fixed sequence: state upload, (max_iteration+1) x [correspondence pass, finalize+solve], result pack
    auto enqueue_all = [&](bool host_checks) -> int {
        // start state and per-hypothesis records: PULLED from the pinned arrays by a kernel, results pushed into the pinned array by one -- no copy
        // command on a per-call path (round 6: the runtime's copy-engine path is where one-off multi-millisecond stalls came from, see drive_host)
        HIP_TRY(prk::launch_stage_words(g->h_dstate.dev, g->dstate.p, sizeof(prk::DevIcpState) * P, g->stream));
        HIP_TRY(prk::launch_stage_words(g->h_meta.dev, g->meta.p, sizeof(prk::PoseMeta) * P, g->stream));
        if (fused) HIP_TRY(prk::launch_fill_i32(g->arrive.as<int32_t>(), P, 0, g->stream));
        auto pass = [&](const prk::IcpBatch &bb, uint32_t p0, uint32_t np, hipStream_t st) -> int {
            if (!timed_call) { HIP_TRY(launch_pass(bb, r.sc, np, st)); return PR_OK; }
            SpanGuard sp(kSpanIcp); HIP_TRY(launch_pass(bb, r.sc, np, st));       // a timed call times every launch of its loop
            uint64_t pts = 0; for (uint32_t i = p0; i < p0 + np; ++i) pts += r.count_h[i];
            g->icp_points += pts; g->icp_bytes += icp_span_bytes(pts, bb.iter == 0 || bb.iter == (uint32_t)r.crit.max_iteration);      // (edge: the first or the score-only last pass)
            return PR_OK;
        };
        // every fourth pass, when the criteria can end a hypothesis early and nothing is being captured: has every hypothesis finished?
        auto after = [&](uint32_t it, bool &stop) -> int {
            if (!(host_checks && may_exit_early && (it & 3) == 3 && it < (uint32_t)r.crit.max_iteration)) return PR_OK;
            for (uint32_t k = 1; k < n_groups; ++k) HIP_TRY(hipStreamSynchronize(g->side[k - 1]));
            HIP_TRY(hipMemcpyAsync(r.h_meta, g->meta.p, sizeof(prk::PoseMeta) * P, hipMemcpyDeviceToHost, g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
            stop = true;
            for (uint32_t i = 0; i < P; ++i) if (r.h_meta[i].state != prk::kSkip) stop = false;
            return PR_OK;
        };
        PR_TRY(device_solve_loop(lanes, n_groups, r.b, P, r.crit, fused, g->meta.as<prk::PoseMeta>(), g->dstate.as<prk::DevIcpState>(), g->arrive.as<uint32_t>(), pass, after));
        HIP_TRY(prk::launch_pack_results(g->dstate.as<prk::DevIcpState>(), dres, P, g->stream));
        // results go to the pinned staging buffer (a pageable destination is not capturable)
        if (r.results_host) HIP_TRY(prk::launch_stage_words64(dres, g->h_results.dev, sizeof(pr_result) * P, g->stream));
        return PR_OK;
    };

    if (opt.use_graph && n_groups == 1 && (opt.profile == 0 || (opt.profile == 2 && !sample_call))) {   // HIP events recorded inside a captured graph cannot be timed
        const prk::IcpBatch &b = r.b;
        GraphKey key;
        key.add(P); key.add(b.nblk); key.add(b.steps); key.add(crit); key.add(r.sc); key.add(b.cloud); key.add(g->meta.p); key.add(g->partial.p);
        key.add(g->dstate.p); key.add(dres); key.add(r.results_host != nullptr); key.add(r.res); key.add(r.h_meta); key.add(init); key.add(opt.profile); key.add(pose_groups_for(r.sc.kind)); key.add(opt.fused_solve); key.add(g->arrive.p); key.add(b.nn_prev);
        key.add(b.nn_slack); key.add(b.nn_queue); key.add(b.nn_queue2); key.add(b.nn_qcount); key.add(b.robust_kind); key.add(b.robust_c); key.add(b.robust_inv_c);    // nn_carve: behind nn_prev at multiples of `span` (max start+count) -- same P / max_n, other offsets => other addresses
        CachedGraph *hit = nullptr;
        PR_TRY(cached_graph(key, [&] { return enqueue_all(/*host_checks=*/false); }, hit));
        HIP_TRY(hipGraphLaunch(hit->exec, g->stream));
        if (hit->nn_pass) { g_nn_lds_nodes.store(hit->nn_lds_nodes); g_nn_stack_depth.store(hit->nn_stack_depth); }
    } else
        PR_TRY(enqueue_all(/*host_checks=*/true));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (r.results_host) std::memcpy(r.results_host, r.res, sizeof(pr_result) * P);
    drain_spans();
    return PR_OK;
}

// ---- PR_SOLVE_HOST: the software pipeline over pose groups ---------------------------------------------------------------------------------
// Per iteration one launch + one small D2H, then the per-pose logic of icp.cu:178-212 on the host.  The batch runs
// as up to four pose groups, each on a stream of its own, software-pipelined: while the host waits for, solves and re-arms one
// group, the correspondence pass of the next group is on the chip -- the host's share of an iteration (copy latency, wake-up,
// 160 ns per 6x6 solve) is as long as the pass itself, and a single group leaves the GPU idle for all of it.  Results per
// hypothesis do not depend on the grouping (sums, solve and state are per hypothesis).  A timed call (profile 1) is one group.
struct HostRun {
    IcpRun &r; uint32_t n_groups; Lanes lanes;
    bool host_fused, poll_flag;
    float *sums_dev;                             // h_sums as the device sees it (host_fused), or null
    const prk::PoseMeta *h_meta_mapped, *meta_dev;      // h_meta as the device sees it; what the passes read their state from (null: g->meta, staged per iteration)
    volatile uint32_t *h_flags;                  // one flag per pose group, behind the sums
    bool sample_call; uint32_t sample_it;        // profile 2: this call times the pass of iteration sample_it
    uint32_t begin(uint32_t grp) const { return group_begin(r.P, n_groups, grp); }
    int enqueue_group(uint32_t grp, uint32_t it) const; bool solve_one(uint32_t i, uint32_t it) const; bool wait_flag(uint32_t grp, uint32_t it) const; int finish_group(uint32_t grp, uint32_t it) const;
};
// one iteration of one group goes onto its stream: state upload, pass, block sums -> pose sums, download
int HostRun::enqueue_group(uint32_t grp, uint32_t it) const
{
    const uint32_t p0 = begin(grp), np = begin(grp + 1) - p0;
    hipStream_t st = lane(lanes, grp);
    prk::IcpBatch whole = r.b;
    if (meta_dev) whole.meta = meta_dev;                         // the pass reads the 64-byte state of its hypothesis from the pinned host array
    else HIP_TRY(prk::launch_stage_words(h_meta_mapped + p0, g->meta.as<prk::PoseMeta>() + p0, sizeof(prk::PoseMeta) * np, st));   // (pulled by a kernel: no copy command per iteration)
    prk::IcpBatch bb = group_slice(whole, p0);
    bb.iter = it;
    if (host_fused) { bb.fused = 2; bb.arrive = g->arrive.as<uint32_t>() + p0; bb.sums_out = sums_dev + (size_t)p0 * prk::kAccStride; }
    if (poll_flag) {                                             // the group's count and flag (see pass_deliver): how many hypotheses will deliver
        uint32_t expected = 0;
        for (uint32_t i = p0; i < p0 + np; ++i) expected += (r.h_meta[i].state != prk::kSkip) ? 1u : 0u;
        bb.grp_count = g->arrive.as<uint32_t>() + r.P + grp; bb.grp_expected = expected;
        bb.grp_flag = reinterpret_cast<uint32_t *>(sums_dev + (size_t)r.P * prk::kAccStride) + grp;
    }
    if (opt.profile == 1 || opt.profile == 3 || (sample_call && it == sample_it)) {
        SpanGuard sp(kSpanIcp); HIP_TRY(launch_pass(bb, r.sc, np, st));
        // (edge: the first pass only -- this loop's last pass is not score-only)
        for (uint32_t i = p0; i < p0 + np; ++i) if (r.h_meta[i].state != prk::kSkip) { g->icp_points += r.count_h[i]; g->icp_bytes += icp_span_bytes(r.count_h[i], it == 0); }
    } else HIP_TRY(launch_pass(bb, r.sc, np, st));
    if (!host_fused) {
        HIP_TRY(prk::launch_icp_finalize(bb.partial, g->meta.as<prk::PoseMeta>() + p0, r.b.nblk, r.b.steps, g->sums.as<float>() + (size_t)p0 * prk::kAccStride, np, st));
        HIP_TRY(hipMemcpyAsync(r.h_sums + (size_t)p0 * prk::kAccStride, g->sums.as<float>() + (size_t)p0 * prk::kAccStride, sizeof(float) * prk::kAccStride * np,
                               hipMemcpyDeviceToHost, st));
    }
    return PR_OK;
}
// the host's part of an iteration for one hypothesis whose 29 sums have arrived (icp.cu:178-212); returns whether the hypothesis goes on
bool HostRun::solve_one(uint32_t i, uint32_t it) const
{
    float E[16];
    if (r.trace.rows) std::memcpy(r.trace.rows + ((size_t)it * r.trace.n_hyp + i) * 29, r.h_sums + (size_t)i * prk::kAccStride, sizeof(float) * 29);   // pr_debug_trace_sums: it < n_passes, i < n_hyp (sums_trace_admits)
    if (!pose_iteration_host(r.h_sums + (size_t)i * prk::kAccStride, r.count_h[i], r.res[i], r.crit, it, E)) { r.h_meta[i].state = prk::kSkip; return false; }
    std::memcpy(r.h_meta[i].xform, E, sizeof(float) * 12);
    r.h_meta[i].state = prk::kRunWithTransform;
    return true;
}
// until the group's flag carries iteration it's tag and every row that was due has arrived; false: a HIP error
bool HostRun::wait_flag(uint32_t grp, uint32_t it) const
{
    hipStream_t st = lane(lanes, grp);
    const uint32_t tag = it + 1u;
    uint32_t idle = 0;
    bool drained = false;
    while (h_flags[grp] != tag) {
        if (drained) { set_error("PR_SOLVE_HOST: the pass of iteration %u ended without completing its pose group", it); return false; }
        if (++idle >= 20000u) {                              // every few hundred microseconds of fruitless polling: is the stream still alive?
            idle = 0;
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) drained = true;           // (one more look: the flag was stored before the kernel ended)
            else if (q != hipErrorNotReady) { (void)hipGetLastError(); set_error("HIP error: %s", hipGetErrorString(q)); return false; }
        }
        cpu_relax();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    // every row that was due carries the iteration's tag behind its sums (pass_deliver): a row without it was overtaken by the flag -- wait for the
    // stream (the end of the launch makes everything visible) instead of solving on stale sums
    bool all_in = true;
#if PR_HOST_ROW_TAG
    for (uint32_t i = begin(grp); i < begin(grp + 1) && all_in; ++i)
        if (r.h_meta[i].state != prk::kSkip && reinterpret_cast<volatile uint32_t *>(r.h_sums + (size_t)i * prk::kAccStride)[31] != tag) all_in = false;
#endif
    if (!all_in) {
        g_flag_overtook.fetch_add(1);
        if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess) { set_error("HIP error: %s", hipGetErrorString(e)); return false; }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return true;
}
// returns how many hypotheses of the group go on; < 0: a HIP error
int HostRun::finish_group(uint32_t grp, uint32_t it) const
{
    if (poll_flag) { if (!wait_flag(grp, it)) return -1; }
    else if (hipError_t e = hipStreamSynchronize(lane(lanes, grp)); e != hipSuccess) { set_error("HIP error: %s", hipGetErrorString(e)); return -1; }
    int active = 0;
    for (uint32_t i = begin(grp); i < begin(grp + 1); ++i) if (r.h_meta[i].state != prk::kSkip && solve_one(i, it)) ++active;
    return active;
}
int drive_host(IcpRun &r)
{
    const uint32_t P = r.P;
    const pr_criteria crit = r.crit;
    // profile 2: one call in sample_period times ONE of its passes (a different iteration from call to call); that call runs as one pose
    // group like the calls of profile 1 / 3, so that the timed launch has the chip to itself -- the other calls keep their pipeline
    const uint64_t host_tick = g->sample_clock++;
    const bool sample_call = (opt.profile == 2) && (host_tick % (uint64_t)std::max(1, opt.sample_period) == 0);
    const uint32_t sample_it = (uint32_t)(((host_tick / (uint64_t)std::max(1, opt.sample_period)) * 5 + 1) % (uint64_t)(crit.max_iteration + 1));
    const uint32_t n_groups = pose_group_count(r.sc.kind, P, opt.profile == 1 || opt.profile == 3 || sample_call);
    const Lanes lanes{ g->stream, g->side, g->ev_fork, g->ev_join };
    if (opt.fused_solve) { PR_TRY(g->arrive.ensure(sizeof(uint32_t) * (P + 4))); HIP_TRY(prk::launch_fill_i32(g->arrive.as<int32_t>(), (size_t)P + 4, 0, g->stream)); }   // (+ one counter per pose group)
    PR_TRY(lanes_fork(lanes, n_groups));                              // the groups start behind the render / cloud work of this call
    // With option fused_solve the pass also adds up the workgroup sums of a hypothesis (the workgroup that arrives last does, as in the
    // device-solve loop) and stores the 29 totals straight into the pinned host array: no finalize launch, no copy command -- two
    // API calls and one copy-engine round trip less per group and iteration on a path that is bound by exactly those.
    const bool host_fused = opt.fused_solve != 0;
    // Projective scenes also read the per-hypothesis state (64 bytes: cloud span, pending update) from the pinned host array instead
    // of receiving it through a copy command: one uniform load per workgroup over the host link, 1.62 -> 1.54 ms per 256-hypothesis
    // batch.  The four kernels of a kd-tree pass have ten times the workgroups; there the copy is cheaper (8.3 against 8.8 ms).
    const prk::PoseMeta *h_meta_mapped = g->h_meta.dev_as<prk::PoseMeta>();
    // Round 6: the host waits for a pose group's FLAG in pinned memory (stored by the workgroup that delivers the group's last
    // hypothesis) instead of for the stream -- it solves while the launch winds down.  Option blocking_wait (several ranks sharing few CPUs) and
    // host_poll = 0 keep the stream wait.
    const HostRun h{ r, n_groups, lanes, host_fused, host_fused && !opt.blocking_wait && opt.host_poll, host_fused ? g->h_sums.dev_as<float>() : nullptr,
                     h_meta_mapped, (host_fused && r.sc.kind != PR_SCENE_NN) ? h_meta_mapped : nullptr,
                     reinterpret_cast<volatile uint32_t *>(r.h_sums + (size_t)P * prk::kAccStride), sample_call, sample_it };
    if (h.poll_flag) { for (int k = 0; k < 4; ++k) h.h_flags[k] = 0u; for (uint32_t i = 0; i < P; ++i) reinterpret_cast<volatile uint32_t *>(r.h_sums + (size_t)i * prk::kAccStride)[31] = 0u; }
    bool live[4] = { false, false, false, false };
    int rc_loop = PR_OK;
    for (uint32_t grp = 0; grp < n_groups && rc_loop == PR_OK; ++grp) {
        for (uint32_t i = h.begin(grp); i < h.begin(grp + 1); ++i) live[grp] |= (r.h_meta[i].state != prk::kSkip);
        if (live[grp]) rc_loop = h.enqueue_group(grp, 0);
    }
    for (uint32_t it = 0; it <= (uint32_t)crit.max_iteration && rc_loop == PR_OK && (live[0] || live[1] || live[2] || live[3]); ++it) {
        for (uint32_t grp = 0; grp < n_groups && rc_loop == PR_OK; ++grp) {
            if (!live[grp]) continue;
            const int active = h.finish_group(grp, it);
            if (active < 0) { rc_loop = PR_ERR_HIP; break; }
            live[grp] = active > 0;
            if (live[grp]) rc_loop = h.enqueue_group(grp, it + 1);                          // it + 1 <= max_iteration: the last iteration leaves nobody active
        }
    }
    for (uint32_t k = 1; k < n_groups; ++k) (void)hipStreamSynchronize(g->side[k - 1]);  // nothing of this call is left on a side stream, error or not
    if (h.poll_flag) (void)hipStreamSynchronize(g->stream);         // (a flag arrives before its pass has formally ended: nothing of this call runs on after it returns)
    trace_mark("icp_drive: host loop done");
    if (rc_loop != PR_OK) { (void)hipStreamSynchronize(g->stream); drain_spans(); return rc_loop; }
    if (r.results_host) std::memcpy(r.results_host, r.res, sizeof(pr_result) * P);
    if (r.results_dev) {
        // the records are PULLED from the pinned array by a kernel, not pushed by a copy command: round 6 traced the one-off stall of the host-solve
        // pipeline (one step of 6.5-8.7 ms among forty of 1.0 ms, PR_TRACE) to this 18 KB hipMemcpyAsync -- some batches into a helper thread's life
        // the runtime spends milliseconds inside it, on both helpers at once (its copy-engine path; the kernels around it take microseconds)
        HIP_TRY(prk::launch_stage_words64(g->h_results.dev, r.results_dev, sizeof(pr_result) * P, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
    }
    drain_spans();
    return PR_OK;
}

// clouds: cloud i = cloud_base[start_h[i] .. start_h[i]+count_h[i]); start and count reach the device with the per-hypothesis records staged here.
// The set-up both drivers share -- workspaces, the batch, the kd-tree workspace, the start records and results -- then the driver of option solve.
int icp_drive(pr_vec3 *cloud_base, const uint32_t *start_h, const uint32_t *count_h, uint32_t P, const SceneSel &sc_in,
              pr_criteria crit, pr_result *results_host, pr_result *results_dev, const pr_robust &robust)
{
    if (P == 0) return PR_OK;
    if (crit.max_iteration < 0) { set_error("max_iteration must be >= 0"); return PR_ERR_INVALID; }
    PR_TRY(sums_trace_admits("icp_drive", P, crit));               // (a recorder that does not fit this batch: refused before anything is launched)
    IcpRun r;
    r.sc = sc_in; r.crit = crit; r.P = P; r.count_h = count_h; r.results_host = results_host; r.results_dev = results_dev;
    r.trace = tl_sums_trace.active;
    SceneSel &sc = r.sc;
    const uint32_t steps = (uint32_t)std::max(1, opt.steps);
    const uint32_t ppb = steps * prk::kPointsPerStep;
    uint32_t max_n = 0;
    for (uint32_t i = 0; i < P; ++i) max_n = std::max(max_n, count_h[i]);
    const uint32_t nblk = (max_n + ppb - 1) / ppb;

    PR_TRY(g->meta.ensure(sizeof(prk::PoseMeta) * P));
    PR_TRY(g->partial.ensure(sizeof(float) * prk::kAccStride * (size_t)std::max(1u, nblk) * P));
    PR_TRY(g->sums.ensure(sizeof(float) * prk::kAccStride * P));
    PR_TRY(g->h_meta.ensure(sizeof(prk::PoseMeta) * P));
    PR_TRY(g->h_sums.ensure(sizeof(float) * prk::kAccStride * P + 64));        // (+ the pose groups' flags, PR_SOLVE_HOST with host_poll)
    PR_TRY(g->h_results.ensure(sizeof(pr_result) * P));

    prk::IcpBatch &b = r.b;
    b.cloud = cloud_base; b.meta = g->meta.as<prk::PoseMeta>(); b.partial = g->partial.as<float>();
    b.nblk = nblk; b.steps = steps;
    b.robust_kind = robust.kind; b.robust_c = robust.c; b.robust_inv_c = robust.inv_c;       // (the entry points have checked the descriptor)
    sc.nn_split = nn_split_for(sc);
    // a robust pass over a kd-tree scene takes the split route wherever the scene allows it, whatever option nn_split says: the winners pass is
    // the one instantiated with the weight (a scene without compact records walks stackless in the pass, launch_icp_pass_nn)
    if (robust.kind != PR_ROBUST_NONE && sc.kind == PR_SCENE_NN && sc.nn.rec32) sc.nn_split = 1u;
    sc.nn_max_points = max_n;
    if (sc.nn_split && opt.nn_count) {                            // instrumented run: kCounterPasses x 8 counters, accumulated until read
        const bool fresh = g->nn_counters.p == nullptr;
        PR_TRY(g->nn_counters.ensure(sizeof(unsigned long long) * 8 * kCounterPasses));
        if (fresh) HIP_TRY(hipMemsetAsync(g->nn_counters.p, 0, sizeof(unsigned long long) * 8 * kCounterPasses, g->stream));
        if ((uint32_t)crit.max_iteration + 1 <= kCounterPasses) sc.nn.counters = g->nn_counters.as<unsigned long long>();
    }
    if (sc.kind == PR_SCENE_NN && sc.nn.rec32 && (opt.nn_seed || sc.nn_split)) {     // winners, indexed like the cloud points
        size_t span = 1;
        for (uint32_t i = 0; i < P; ++i) span = std::max(span, (size_t)start_h[i] + count_h[i]);
        const NNLayout nl = nn_layout(span, P);
        PR_TRY(g->nn_prev.ensure(nl.bytes));
        nn_carve(b, g->nn_prev.as<uint32_t>(), nl);
        HIP_TRY(prk::launch_fill_i32(reinterpret_cast<int32_t *>(b.nn_qcount), (size_t)prk::kQCountStride * P, 0, g->stream));     // (a kernel, not a memset command: no runtime copy / fill path on a per-call path, see drive_host)
    }

    r.h_meta = g->h_meta.as<prk::PoseMeta>(); r.h_sums = g->h_sums.as<float>(); r.res = g->h_results.as<pr_result>();
    for (uint32_t i = 0; i < P; ++i) {
        identity16(r.res[i].T); r.res[i].inlier_rmse = 0.0f; r.res[i].fitness = 0.0f;   // icp.h:29-31
        std::memset(&r.h_meta[i], 0, sizeof(prk::PoseMeta));
        r.h_meta[i].start = start_h[i]; r.h_meta[i].count = count_h[i];
        r.h_meta[i].state = (count_h[i] > 0) ? prk::kRun : prk::kSkip;    // empty cloud: count==0 -> identity result (icp.cu:183)
    }
    return opt.solve_mode == PR_SOLVE_DEVICE ? drive_device(r) : drive_host(r);
}

}  // namespace prr

using namespace prr;

// pr_icp_batch and pr_icp_batch_robust (fn: whose messages) behind the latter's descriptor check
static int icp_batch_impl(const char *fn, pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                          pr_criteria crit, const pr_robust &robust, pr_result *results_host)
{
    TraceScope traced;                                            // (pr_debug_trace_sums: this call and no other)
    PR_ENTER();
    if (!offsets_host || (n_clouds && !results_host)) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    if (n_clouds == 0) return PR_OK;
#ifndef PR_MAX_CLOUDS_PER_RUN
#define PR_MAX_CLOUDS_PER_RUN 32768                               // (a larger value in an experiment build exercises the launchers' own split)
#endif
    constexpr uint32_t kMaxCloudsPerRun = PR_MAX_CLOUDS_PER_RUN;
    PR_TRY(sums_trace_admits(fn, n_clouds, crit));     // (pr_debug_trace_sums: the whole list against the recorder, before the scene is touched)
    if (tl_sums_trace.active.rows && n_clouds > kMaxCloudsPerRun) { set_error("%s: pr_debug_trace_sums records one run of at most %u clouds, the list has %u", fn, kMaxCloudsPerRun, n_clouds); return PR_ERR_INVALID; }
    if (!clouds_dev) {                                            // clouds without a single point come without an array (an empty device_vector):
        if (offsets_host[n_clouds] != offsets_host[0]) { set_error("%s: null cloud array", fn); return PR_ERR_INVALID; }
        for (uint32_t i = 0; i < n_clouds; ++i) {                 // count == 0 -> identity, fitness 0, rmse 0 (icp.cu:183), like any empty cloud
            identity16(results_host[i].T); results_host[i].fitness = 0.0f; results_host[i].inlier_rmse = 0.0f;
        }
        return PR_OK;
    }
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(scene_kind, scene, /*want_packed=*/false, sc));
    std::vector<uint32_t> start(n_clouds), count(n_clouds);
    for (uint32_t i = 0; i < n_clouds; ++i) {
        if (offsets_host[i + 1] < offsets_host[i]) { set_error("%s: offsets must be non-decreasing", fn); return PR_ERR_INVALID; }
        start[i] = offsets_host[i]; count[i] = offsets_host[i + 1] - offsets_host[i];
    }
    // the hypothesis index is the y dimension of every launch of the loop (65 535 at most): longer lists run in pieces, one after the other
    // (the clouds are independent of each other, so the pieces are)
    for (uint32_t c0 = 0; c0 < n_clouds; c0 += kMaxCloudsPerRun) {
        const uint32_t nc = std::min(kMaxCloudsPerRun, n_clouds - c0);
        PR_TRY(icp_drive(clouds_dev, start.data() + c0, count.data() + c0, nc, sc, crit, results_host + c0, nullptr, robust));
    }
    return PR_OK;
}

extern "C" {

int pr_icp_batch(pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                 pr_criteria crit, pr_result *results_host)
{
    return icp_batch_impl("pr_icp_batch", clouds_dev, offsets_host, n_clouds, scene_kind, scene, crit, pr_robust{ PR_ROBUST_NONE, 0.0f, 0.0f, 0 }, results_host);
}

int pr_robust_describe(uint32_t kind, float c, pr_robust *out)
{
    const char *fn = "pr_robust_describe";
    if (!out) { set_error("%s: bad arguments (out is null)", fn); return PR_ERR_INVALID; }
    pr_robust rb{ kind, kind == PR_ROBUST_NONE ? 0.0f : c, 0.0f, 0 };
    if (kind != PR_ROBUST_NONE && kind <= PR_ROBUST_CAUCHY && std::isfinite(c) && c > 0.0f) rb.inv_c = 1.0f / c;     // once, in float32
    PR_TRY(robust_desc_ok(fn, &rb));
    *out = rb;
    return PR_OK;
}

int pr_icp_batch_robust(pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                        pr_criteria crit, const pr_robust *robust, pr_result *results_host)
{
    PR_TRY(robust_desc_ok("pr_icp_batch_robust", robust));          // before any device is touched
    if (!offsets_host || (n_clouds && (!results_host || !scene))) { set_error("pr_icp_batch_robust: bad arguments"); return PR_ERR_INVALID; }
    return icp_batch_impl("pr_icp_batch_robust", clouds_dev, offsets_host, n_clouds, scene_kind, scene, crit, *robust, results_host);
}

int pr_icp_proj(pr_vec3 *cloud_dev, uint32_t n_points, const pr_scene_proj *scene, pr_criteria crit, pr_result *result_out)
{
    const uint32_t off[2] = { 0, n_points };
    return pr_icp_batch(cloud_dev, off, 1, PR_SCENE_PROJ, scene, crit, result_out);
}

int pr_icp_nn(pr_vec3 *cloud_dev, uint32_t n_points, const pr_scene_nn *scene, pr_criteria crit, pr_result *result_out)
{
    const uint32_t off[2] = { 0, n_points };
    return pr_icp_batch(cloud_dev, off, 1, PR_SCENE_NN, scene, crit, result_out);
}

int pr_icp_grid(pr_vec3 *cloud_dev, uint32_t n_points, const pr_scene_grid *scene, pr_criteria crit, pr_result *result_out)
{
    const uint32_t off[2] = { 0, n_points };
    return pr_icp_batch(cloud_dev, off, 1, PR_SCENE_GRID, scene, crit, result_out);
}

// Audit entry: the 29 sums of every pass of the calling thread's NEXT synchronous ICP call (pr_icp_batch / pr_icp_proj / pr_icp_nn / pr_refine_batch[_roi]), as
// the host-solve loop received them -- HostRun::solve_one copies the row of hypothesis i at iteration it to rows_host[(it * n_hyp + i) * 29 ..] right before
// pose_iteration_host consumes it, whichever way the sums came (pinned-memory stores of the pass tail, finalize launch + copy, flag polling or stream
// wait, any pose grouping).  Rows of skipped or finished hypotheses are left alone.  NULL disarms.  Host code only: no device needed to arm.
int pr_debug_trace_sums(float *rows_host, uint32_t n_hyp, uint32_t n_passes)
{
    tl_sums_trace.armed = SumsTrace();
    if (!rows_host) return PR_OK;
    if (n_hyp == 0 || n_passes == 0) { set_error("pr_debug_trace_sums: n_hyp and n_passes must be positive"); return PR_ERR_INVALID; }
    tl_sums_trace.armed = SumsTrace{ rows_host, n_hyp, n_passes };
    return PR_OK;
}

// Audit entry: what ONE correspondence pass contributes, point by point (29 floats each: the 21 upper-triangle products of J J^T row by
// row, the 6 products J r, r^2 and the inlier flag -- thrust__pcd2Ab, icp.h:128-209), with the pending update applied to the cloud first
// like the fused pass does.  A caller that adds the rows in point order reproduces the reference's single-thread sums (icp.cpp:139-148).
int pr_debug_contrib29(pr_vec3 *cloud_dev, uint32_t n_points, int scene_kind, const void *scene, const float *update16, int want_packed, float *contrib_host)
{
    PR_ENTER();
    if (n_points == 0) return PR_OK;
    if (!cloud_dev || !contrib_host) { set_error("pr_debug_contrib29: null buffer"); return PR_ERR_INVALID; }
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(scene_kind, scene, want_packed != 0, sc));
    DevBuf out;
    PR_TRY(out.ensure(sizeof(float) * 29 * (size_t)n_points));
    hipError_t e;
    if (sc.kind == PR_SCENE_GRID) e = prk::launch_contrib29_grid(cloud_dev, n_points, update16, sc.grid, out.as<float>(), g->stream);
    else if (sc.kind == PR_SCENE_NN) e = prk::launch_contrib29_nn(cloud_dev, n_points, update16, sc.nn, out.as<float>(), g->stream);
    else if (sc.packed) e = prk::launch_contrib29_proj_packed(cloud_dev, n_points, update16, sc.pk, out.as<float>(), g->stream);
    else e = prk::launch_contrib29_proj_aos(cloud_dev, n_points, update16, sc.aos, out.as<float>(), g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(contrib_host, out.p, sizeof(float) * 29 * (size_t)n_points, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    note_write(cloud_dev, sizeof(pr_vec3) * (size_t)n_points);
    out.release();
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("pr_debug_contrib29: %s", hipGetErrorString(e)); return PR_ERR_HIP; }
    return PR_OK;
}

// Audit entry: pr_debug_contrib29 with the weighted terms of `robust`, and per point the correspondence and weight beside them (corr_host, optional).
int pr_debug_robust_terms(pr_vec3 *cloud_dev, uint32_t n_points, int scene_kind, const void *scene, const float *update16, int want_packed,
                          const pr_robust *robust, float *contrib_host, float *corr_host)
{
    PR_TRY(robust_desc_ok("pr_debug_robust_terms", robust));        // before any device is touched
    if (n_points && (!cloud_dev || !contrib_host || !scene)) { set_error("pr_debug_robust_terms: null buffer"); return PR_ERR_INVALID; }
    PR_ENTER();
    if (n_points == 0) return PR_OK;
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(scene_kind, scene, want_packed != 0, sc));
    DevBuf out;
    const size_t b_terms = sizeof(float) * 29 * (size_t)n_points, b_corr = corr_host ? sizeof(float) * 8 * (size_t)n_points : 0;
    PR_TRY(out.ensure(((b_terms + 15) & ~(size_t)15) + b_corr));
    float *d_corr = corr_host ? reinterpret_cast<float *>(static_cast<char *>(out.p) + ((b_terms + 15) & ~(size_t)15)) : nullptr;      // (16-byte aligned: the rows go out as float4)
    const prk::RobustArgs ra{ robust->kind, robust->c, robust->inv_c, d_corr };
    hipError_t e;
    if (sc.kind == PR_SCENE_GRID) e = prk::launch_robust_terms_grid(cloud_dev, n_points, update16, sc.grid, ra, out.as<float>(), g->stream);
    else if (sc.kind == PR_SCENE_NN) e = prk::launch_robust_terms_nn(cloud_dev, n_points, update16, sc.nn, ra, out.as<float>(), g->stream);
    else if (sc.packed) e = prk::launch_robust_terms_proj_packed(cloud_dev, n_points, update16, sc.pk, ra, out.as<float>(), g->stream);
    else e = prk::launch_robust_terms_proj_aos(cloud_dev, n_points, update16, sc.aos, ra, out.as<float>(), g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(contrib_host, out.p, b_terms, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess && corr_host) e = hipMemcpyAsync(corr_host, d_corr, b_corr, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    note_write(cloud_dev, sizeof(pr_vec3) * (size_t)n_points);
    out.release();
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("pr_debug_robust_terms: %s", hipGetErrorString(e)); return PR_ERR_HIP; }
    return PR_OK;
}

// Audit entry: one iteration of icp.cu:178-212 on given sums, through the device's wavefront iteration (icp_solve_device.h, what the
// fused pass tail and icp_finalize_solve_kernel run) or through the host-solve loop's pose_iteration_host.
int pr_debug_pose_iteration(const float *sums, const uint32_t *n_points, uint32_t n, pr_criteria crit, uint32_t iter, int on_device,
                            pr_result *state, float *update_out, uint32_t *finished_out)
{
    if (n == 0) return PR_OK;
    if (!sums || !n_points || !state || !update_out || !finished_out) { set_error("pr_debug_pose_iteration: null buffer"); return PR_ERR_INVALID; }
    if (!on_device) {                                            // host code only: no device needed
        for (uint32_t i = 0; i < n; ++i) {
            float E[16];
            const bool go_on = pose_iteration_host(sums + (size_t)i * 29, n_points[i], state[i], crit, iter, E);
            for (int k = 0; k < 16; ++k) update_out[(size_t)i * 16 + k] = go_on ? E[k] : 0.0f;
            finished_out[i] = go_on ? 0u : 1u;
        }
        return PR_OK;
    }
    PR_ENTER();
    const size_t b_sums = sizeof(float) * 29 * n, b_cnt = sizeof(uint32_t) * n, b_st = sizeof(pr_result) * n, b_upd = sizeof(float) * 16 * n;
    DevBuf buf;
    PR_TRY(buf.ensure(b_sums + b_cnt + b_st + b_upd + b_cnt));
    char *base = static_cast<char *>(buf.p);
    float *d_sums = reinterpret_cast<float *>(base);
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(base + b_sums);
    pr_result *d_st = reinterpret_cast<pr_result *>(base + b_sums + b_cnt);
    float *d_upd = reinterpret_cast<float *>(base + b_sums + b_cnt + b_st);
    uint32_t *d_fin = reinterpret_cast<uint32_t *>(base + b_sums + b_cnt + b_st + b_upd);
    hipError_t e = hipMemcpyAsync(d_sums, sums, b_sums, hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cnt, n_points, b_cnt, hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_st, state, b_st, hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) e = prk::launch_pose_iteration_debug(d_sums, d_cnt, n, crit, iter, d_st, d_upd, d_fin, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(state, d_st, b_st, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(update_out, d_upd, b_upd, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(finished_out, d_fin, b_cnt, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    buf.release();
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("pr_debug_pose_iteration: %s", hipGetErrorString(e)); return PR_ERR_HIP; }
    return PR_OK;
}

// work counters of the kd-tree search kernel (option "nn_count"): out[pass * 8 + k], k = queries, settled by the pixel window,
// handed to the tree, pyramid descents, tree nodes visited, leaves scanned, leaf points tested, window cells read; reading resets them
int pr_nn_counters(uint64_t *out, uint32_t passes)
{
    PR_ENTER();
    if (!out || passes == 0 || passes > kCounterPasses) { set_error("pr_nn_counters: bad arguments"); return PR_ERR_INVALID; }
    std::memset(out, 0, sizeof(uint64_t) * 8 * passes);
    if (!g->nn_counters.p) return PR_OK;
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(out, g->nn_counters.p, sizeof(uint64_t) * 8 * passes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(g->nn_counters.p, 0, sizeof(unsigned long long) * 8 * kCounterPasses));
    return PR_OK;
}

}  // extern "C"
