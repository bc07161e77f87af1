#!/usr/bin/env python
"""bench.py -- refined poses/s of the fused hot path (render -> cloud -> 21-pass ICP) on N MI355X.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic hypotheses per GPU:
BASELINE.json configs[1] -- obj_06.ply, 256-pose batch, 640x480, projective association,
ICPConvergenceCriteria(0,0,20) => exactly 21 correspondence passes / 20 solves per pose
(SURVEY.md 8d).  Model triangles and the scene are resident in HBM before the timed region; the
timed region includes the pose upload (64 B/pose), every kernel, the per-iteration host solve
round trips (PR_SOLVE_HOST) or the device solve, and the result gather.

Multi-GPU: the global batch is cut into contiguous shards (pr_shard_range), rank r refines its shard of
the seeded stream -- no data-path collective -- then ONE RCCL gather of the 72-byte RegistrationResult
records to rank 0 over xGMI: pr_gather_results of the C ABI (grouped ncclSend/ncclRecv on the library's
stream; the communicator's 128-byte id travels over torch.distributed, which also provides the barrier
and the max-over-ranks clock).  PR_BENCH_GATHER=torch uses torch.distributed.gather instead.
  --scaling weak   (default) per-GPU batch fixed: --poses 256 per GPU, or --global-poses G / N
  --scaling strong the global batch is fixed (--global-poses, default 4096 = BASELINE configs[3]) and split over the N ranks
      python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
             bench.py --gpus 8 --global-poses 4096          # configs[3]: 512 hypotheses per GPU

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).
A plain run sets up, runs W warm-up and K timed steps and prints the line, nothing else.
  --full              everything else as well: `roofline` for the dominant kernel (the correspondence kernel,
                      HIP-event timed on the library's own stream, one more untimed step; live rocprofv3 counter
                      passes), the other configurations (kd-tree, host solve, default criteria, a new scene per
                      frame, BASELINE configs[3] / [4]) and `cpu_baseline` (the CPU oracle on a bounded sample,
                      rank 0, N=1 only)
  --dump-outputs DIR  after the timed steps, what the last timed step returned to its caller (rank 0's records and
                      cloud sizes) as DIR/<name>.npy: T (P x 16), fitness, inlier_rmse (float32), sizes (float64)
"""
import argparse
import json
import os
import sys
import time

# The pipelined loop keeps four streams busy side by side (two slots x two pose groups).  The HIP runtime maps every stream of
# the process onto GPU_MAX_HW_QUEUES hardware queues (default 4, shared with torch's and RCCL's streams) and streams that share
# a queue serialise, so ask for 16 (the slots' four, a third pose group for kd-tree scenes, the private contexts of the host-solve threads, torch's
# and RCCL's own) -- before torch initialises the runtime.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                       # MI355X_MICROARCH.md: 8 TB/s spec
# VALU issue peak, CALIBRATED (round 6): tools/valu_peak.hip -> profiles/r06/valu_peak.md.  Chains of independent non-packed
# v_mul_f32 / v_add_f32 / v_fma_f32 / v_add_u32 over all 256 CUs retire 0.98-1.02e12 wave-instructions/s from two resident wavefronts per SIMD on
# (= 1024 SIMDs x 2.4 GHz / 2.4-2.5 cycles: the guide's "a wave64 VALU instruction issues over 2 cycles", MI355X_MICROARCH.md:52-54, at the clock the
# chip holds under that load); ONE wavefront per SIMD gets 0.47e12 (a wavefront issues a VALU instruction every ~4.75 cycles).  Half of that rate:
# v_pk_*_f32, v_fma_f64, DPP forms, v_cvt_*, v_min3_u32, v_mul_lo_u32 (0.52-0.60e12); a quarter: v_rcp_f32 / v_sqrt_f32 (0.30e12).  Rounds 4-5 assumed
# 6.14e11 (one instruction per 4 cycles) and called kernels at 0.5-0.75 of it VALU-bound; against the measured peak they sit at 0.3-0.45.
VALU_PEAK = 0.977e12
VALU_PEAK_SOURCE = ("profiles/r06/valu_peak.md (tools/valu_peak.hip on this pool's MI355X: v_mul_f32 chains, 8 wavefronts per SIMD, 0.977e12 wave-instructions/s; "
                    "packed-f32 / f64 / DPP / cvt forms 0.52-0.60e12, transcendentals 0.30e12)")
# SURVEY.md 8d algorithmic bytes of the correspondence kernel: per pass 12 B source read + 24 B
# destination/normal gather, + 12 B write-back on every pass after the first:
# N*(21*36 + 20*12) = 996 N bytes per pose over 21 launches.
BYTES_PER_POINT_PASS0, BYTES_PER_POINT_PASSK = 36.0, 48.0
# Committed rocprofv3 PMC measurements of the correspondence kernel: the fallback of live_pmc_traffic(), which collects the same two counters in
# child passes of this run (counters need rocprofv3 passes
# of their own): fabric-side bytes per point (FETCH_SIZE x2 per the gfx950 correction of MI355X_MICROARCH.md + WRITE_SIZE, both calibrated on
# max2zero_kernel, which moves a known number of bytes) and VALU wave-instructions per point (SQ_INSTS_VALU).  FETCH_SIZE counts what the
# L2s fetch from the fabric, Infinity-Cache hits included (guide, HBM section): the counter figure is FABRIC traffic, an upper bound of DRAM
# traffic -- with <= 512 hypotheses per sub-batch the clouds are Infinity-Cache resident by design.
PMC_TRAFFIC_BYTES_PER_POINT = {"proj": 25.1, "nn": 70.9}       # P = 1024 as ONE sub-batch (clouds spill the Infinity Cache): 23.9 B/point -- the same: it is the cloud read + write-back
PMC_VALU_WAVE_INSTR_PER_POINT = {"proj": 2.077, "nn": None}             # profiles/r06: 735 215 064 wave-instructions over 63 launches of 5 618 880 points (740 442 795 before the write-back moved behind the gathers)
# what DRAM carries when the clouds do NOT fit the Infinity Cache (1024 hypotheses as one sub-batch): committed fallback of the run's own passes
PMC_DRAM_FRAC = {"proj": 0.52, "nn": None}
PMC_DRAM_SOURCE = "committed: profiles/r06/pmc_proj_p1024_onebatch_*.md + kernel_stats_p1024_onebatch.md (23.8 B/point x 22.47 M points = 536 MB per 129.2 us launch = 4.15 TB/s)"
# committed SQ counter passes of the kd-tree task walk, pass 0 (profiles/r06/sq_nn_pass0.txt, unchanged from r05's): SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES = the share of a
# wavefront's resident cycles with one of its VALU instructions in flight (six wavefronts share a SIMD), and 4 x SQ_ACTIVE_INST_VALU over
# (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs) = the share of the chip's VALU issue slots the kernel fills
NN_WALK_VALU_ACTIVE_FRAC = 0.21
NN_WALK_VALU_ISSUE_FRAC = 0.75 * 6.144e11 / VALU_PEAK              # r05's 0.75 was against 6.14e11/s: 0.47 of the calibrated peak
# committed SQ pass of the projective correspondence kernel (profiles/r06/sq_proj_SQ_ACTIVE_INST_VALU_SQ_WAVE_CYCLES_SQ_WAIT_INST_ANY.md): share of a
# wavefront's resident cycles spent waiting for an instruction's operands (SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES)
PROJ_PASS_WAIT_FRAC = 0.317
NN_WALK_HBM_BYTES_PER_POINT = 4.6                                  # profiles/r06/pmc_nn_*.md (2 x 589 970 + 428 381 KB over 63 passes of 5.62 M points): the walk reads queue entries + cloud points, writes winners
PMC_TRAFFIC_SOURCE = {"proj": "profiles/r06/pmc_proj_FETCH_SIZE.md + pmc_proj_WRITE_SIZE.md + sq_proj_SQ_INSTS_VALU*.md (icp_pass_kernel<SceneProjPacked>)",
                      "nn": "profiles/r06/pmc_nn_FETCH_SIZE.md + pmc_nn_WRITE_SIZE.md (search 37.1 + bound 11.2 + task walk 4.6 + winners pass 17.9 B/point)"}


def effective_cpus():
    """CPUs this process may really use: the affinity mask, capped by the cgroup CPU quota (cpu.max: a box with 256 online CPUs and a
    quota of 16 runs 256 OpenMP threads on 16 CPUs' worth of time).  Returns (usable, facts)."""
    facts = {"online": os.cpu_count(), "affinity": len(os.sched_getaffinity(0))}
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        facts["cgroup_cpu_max"] = f"{q} {per}"
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            facts["cgroup_cfs"] = f"{q} {per}"
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    usable = facts["affinity"]
    if quota is not None:
        usable = max(1, min(usable, int(quota + 0.5)))
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                facts["model"] = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return usable, facts


def flush_c_stdio():
    """RCCL prints its version banner through C stdio when NCCL_DEBUG=VERSION (set in this image); with stdout redirected that text sits in a
    C buffer until the process exits -- i.e. it would land AFTER the JSON line.  Flushing it when it is written keeps the JSON line last."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:                                              # noqa: BLE001
        pass


# ---- the job's control plane: barrier, max over ranks, small objects to everybody ------------------------------------------------
class SoloGroup:
    """One rank."""
    world, rank, kind = 1, 0, "solo"

    def barrier(self):
        pass

    def all_gather(self, obj):
        return [obj]

    def destroy(self):
        pass


class TorchGroup:
    """One process per GPU (the contract's launch): torch.distributed on RCCL, gloo when the ranks share one device (test mode)."""
    kind = "processes"

    def __init__(self, rank, world, local_rank, share_device):
        import torch
        import torch.distributed as dist
        self.dist, self.world, self.rank = dist, world, rank
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                                               # PR_BENCH_FORCE_COMM=1 without a launcher around it: a rendezvous of one
            os.environ.setdefault("MASTER_PORT", str(free_port()))
        if share_device:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    def barrier(self):
        self.dist.barrier()

    def all_gather(self, obj):
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out

    def destroy(self):
        self.dist.barrier()
        self.dist.destroy_process_group()


class ThreadGroup:
    """One process, one host thread per GPU (SURVEY 8e's launcher-free form, tests/cpp/shard_test.cpp in C++): the ranks meet at a
    threading.Barrier and exchange small objects through a shared list."""
    kind = "threads"

    class Shared:
        def __init__(self, world):
            import threading
            self.world, self.bar, self.box = world, threading.Barrier(world), [None] * world

    def __init__(self, shared, rank):
        self.sh, self.world, self.rank = shared, shared.world, rank

    def barrier(self):
        self.sh.bar.wait()

    def all_gather(self, obj):
        self.sh.box[self.rank] = obj
        self.sh.bar.wait()
        out = list(self.sh.box)
        self.sh.bar.wait()
        return out

    def destroy(self):
        pass


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="ranks of the job, one per GPU.  Without WORLD_SIZE in the environment and N > 1 this process "
                                                          "starts the N ranks itself (--launcher)")
    ap.add_argument("--launcher", choices=["processes", "threads"], default=os.environ.get("PR_BENCH_LAUNCHER", "processes"),
                    help="how `bench.py --gpus N` (N > 1, no WORLD_SIZE) starts its ranks: processes = re-run under torch.distributed.run "
                         "(one process per GPU, the contract's form); threads = one process, one host thread per GPU, pr_comm_init_all")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--poses", type=int, default=256, help="hypotheses per GPU per step (weak scaling)")
    ap.add_argument("--global-poses", type=int, default=0, help="hypotheses per step over ALL GPUs (0: --poses x GPUs); BASELINE configs[3] = 4096 on 8 GPUs")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: per-GPU batch fixed (--poses, or --global-poses / N); strong: the global batch is fixed (--global-poses, default 4096) and split over the ranks")
    ap.add_argument("--gather", choices=["job", "step"], default="job",
                    help="N > 1: job = ONE exchange of all K x P result records after the last step (north_star's single gather); step = one exchange per step, under the next step")
    ap.add_argument("--no-config3", action="store_true", help="N > 1: skip the BASELINE configs[3] measurement (4096 hypotheses over the N ranks) appended to the line")
    ap.add_argument("--scene", choices=["proj", "nn"], default="proj")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--solve", choices=["host", "device"], default=os.environ.get("PR_BENCH_SOLVE", "device"))
    ap.add_argument("--pose-groups", type=int, default=0, help="streams the iteration loop is split over (0 = the library's choice: 2)")
    ap.add_argument("--fused-solve", type=int, default=1, help="1: finalize+solve in the tail of the pass kernel (library default)")
    ap.add_argument("--overlap-pass", type=int, default=-1, help="library option overlap_pass (-1: library default)")
    ap.add_argument("--sequential", action="store_true",
                    help="every step through the synchronous single-group path with HIP events around EVERY correspondence launch "
                         "(profile 1): the mode in which rocprofv3's per-launch average and the event average measure the same thing")
    ap.add_argument("--sample-in", choices=["after", "warmup", "timed"], default=None,
                    help="where the roofline sample (one step with HIP events around every correspondence launch, its loop alone on the chip) is taken: "
                         "after = one more, untimed step behind the closing fence of the timed region (default with --full: the timed region holds pipelined steps only and "
                         "the device is as warm as it gets); warmup = the last warm-up step; timed = the last step of the timed region (rounds 1-3).  "
                         "Without --full and without this option no sample is taken and the line has no `roofline`")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE", help="library option (pr_set_option), repeatable -- tuning runs")
    ap.add_argument("--blocking-wait", type=int, default=-1, help="1: pr_refine_wait sleeps instead of spinning (default: 1 when more than one rank shares the host, else 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--burn-in", type=int, default=0, help="experiments: untimed steps BEFORE the --warmup steps (device clocks up from idle; reported as burn_in_steps).  Default 0: W warm-up steps, K timed steps, nothing else")
    ap.add_argument("--no-live-pmc", action="store_true", help="roofline.traffic from the committed counter passes instead of rocprofv3 --pmc passes run by this process (rank 0, N = 1)")
    ap.add_argument("--no-kdtree-extra", action="store_true", help="skip the short configs[2] (kd-tree association) measurement appended to the line")
    ap.add_argument("--cpu-poses", type=int, default=0, help="CPU baseline sample size (0 = auto)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline too: the roofline sample and live counter passes, the other configurations "
                         "(configs[2] kd-tree, host solve, default criteria, new scene per frame, configs[3] / [4]) and the CPU baseline.  "
                         "Off: the run does only what `value` / `ms_per_step` need")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0: T, fitness, inlier_rmse, sizes) to DIR/<name>.npy")
    return ap.parse_args(argv)


def visible_devices():
    """GPUs this process can see (through the library: pr_device_count; no torch needed)."""
    from pose_refine_amd import api
    return int(api.device_count())


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def check_device_budget(n_ranks, n_visible, share_device):
    """`--gpus N` needs N devices -- unless PR_BENCH_SHARE_DEVICE=1 (test mode for one-GPU boxes: every rank on device 0)."""
    if n_ranks > n_visible and not share_device:
        raise SystemExit(f"bench.py --gpus {n_ranks}: only {n_visible} GPU(s) visible.  Run on a node with {n_ranks} GPUs, or set PR_BENCH_SHARE_DEVICE=1 "
                         "(test mode: every rank uses device 0 and the gather runs on host copies) to exercise the N > 1 path on this box.")


def launch_command(n_ranks, port, argv):
    """The contract's launch line for N ranks on one node, for `bench.py <argv>`."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def has_result_line(text):
    return any(l.startswith('{"metric"') for l in text.splitlines())


def spawn_processes(args, argv):
    """`python bench.py --gpus N` with no WORLD_SIZE: start the N ranks (one process per GPU) under torch.distributed.run and pass their
    line through.  If that launch produces no line (no free port, torchrun missing, a rendezvous failure), the same job is run as N host
    threads of this process (--launcher threads) and the line says so."""
    import subprocess
    cmd = launch_command(args.gpus, free_port(), argv)
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "1")
    env["PR_BENCH_LAUNCHED_BY"] = "bench.py (torch.distributed.run started by `bench.py --gpus N`)"
    print("[bench] starting", " ".join(cmd[1:8]), "...", file=sys.stderr, flush=True)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode == 0 and has_result_line(r.stdout):
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        return 0
    sys.stderr.write(r.stdout)
    print(f"[bench] torch.distributed.run ended with code {r.returncode} and no result line; running the {args.gpus} ranks as host threads of this process", file=sys.stderr, flush=True)
    return run_threads(args, note=f"torch.distributed.run failed (exit code {r.returncode}); fell back to --launcher threads")


def run_threads(args, note=None):
    """One process, one host thread per GPU: pr_comm_init_all(N), pr_set_device(d) per thread, contiguous shards, pr_gather_results."""
    import threading
    import torch                                                    # noqa: F401 -- first, so that torch's HIP runtime is the one in the process
    from pose_refine_amd import api
    n = args.gpus
    share_device = os.environ.get("PR_BENCH_SHARE_DEVICE", "0") == "1"
    check_device_budget(n, visible_devices(), share_device)
    api.init(0)
    comm_note = None
    if not share_device and os.environ.get("PR_BENCH_GATHER", "cabi") != "host":
        try:
            api.comm_init_all(n)                                    # ncclCommInitAll: one communicator per device context
        except Exception as e:                                      # noqa: BLE001 -- the measurement goes on with a host gather
            comm_note = f"pr_comm_init_all({n}) failed: {e}"
    shared = ThreadGroup.Shared(n)
    outs, errs = [None] * n, [None] * n

    def work(rank):
        try:
            outs[rank] = run_rank(args, ThreadGroup(shared, rank), local_dev=0 if share_device else rank, share_device=share_device,
                                  launcher_note=note, comm_ready=(comm_note is None and not share_device), comm_note=comm_note)
        except BaseException as e:                                  # noqa: BLE001
            import traceback
            errs[rank] = "".join(traceback.format_exception(type(e), e, e.__traceback__))
            shared.bar.abort()
    ts = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    bad = [e for e in errs if e and "BrokenBarrierError" not in e] or [e for e in errs if e]
    if bad:
        sys.stderr.write(bad[0])
        return 1
    flush_c_stdio()
    print(json.dumps(outs[0]), flush=True)
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:            # `python bench.py --gpus N`: this process starts the ranks
        if args.launcher == "threads":
            return run_threads(args)
        check_device_budget(args.gpus, visible_devices(), os.environ.get("PR_BENCH_SHARE_DEVICE", "0") == "1")
        return spawn_processes(args, argv)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and "WORLD_SIZE" in os.environ and world > 1:
        print(f"[bench] --gpus {args.gpus} but WORLD_SIZE = {world}: the launcher's world size is used", file=sys.stderr, flush=True)
    # PR_BENCH_FORCE_COMM=1 (test mode for one-GPU boxes): run the whole N > 1 machinery -- process group on the RCCL backend, C-ABI communicator,
    # the gather -- with a world of ONE rank, so that torch's RCCL and the library's use of it meet in one process
    multi = world > 1 or os.environ.get("PR_BENCH_FORCE_COMM", "0") == "1"
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch                                                    # torch first: its bundled HIP runtime must be the one both torch and libpose_refine_hip.so use
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    # PR_BENCH_SHARE_DEVICE=1 is a TEST mode for boxes with one GPU: every rank uses device 0 and the gather runs over
    # gloo on host copies (RCCL refuses two ranks on one device); everything else is the real N>1 code path.
    share_device = os.environ.get("PR_BENCH_SHARE_DEVICE", "0") == "1"
    if share_device:
        local_rank = 0
    if multi and not share_device and local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: local rank {local_rank} but only {torch.cuda.device_count()} GPU(s) visible (PR_BENCH_SHARE_DEVICE=1 lets ranks share device 0: test mode)")
    torch.cuda.set_device(local_rank)
    group = TorchGroup(rank, world, local_rank, share_device) if multi else SoloGroup()
    out = run_rank(args, group, local_dev=local_rank, share_device=share_device, launcher_note=None, comm_ready=False, comm_note=None, force_multi=multi)
    if out is not None:
        flush_c_stdio()
        print(json.dumps(out), flush=True)
    group.destroy()
    return 0


def run_rank(args, group, local_dev, share_device, launcher_note, comm_ready, comm_note, force_multi=False):
    """Everything one rank does; rank 0 returns the line (a dict), the others None."""
    import numpy as np
    from pose_refine_amd import api, synth
    from pose_refine_amd import dist as prd

    world, rank = group.world, group.rank
    multi = world > 1 or force_multi
    threads_mode = group.kind == "threads"
    if threads_mode:
        api.set_device(local_dev)
        if share_device:
            api.thread_context(True)                                # ranks sharing device 0: a private context (stream, workspaces, slots) each
    else:
        api.init(local_dev)
    # the gather of the solved transforms: C ABI (RCCL directly) unless told otherwise or the communicator cannot be formed;
    # ranks that share one device (test mode) exchange host copies through the control plane
    want = os.environ.get("PR_BENCH_GATHER", "cabi")
    # PR_RCCL_LIBRARY = the loop-back stand-in (tests/rccl_loopback: ranks of ONE process matched through a table): rank THREADS that share device 0
    # then gather through pr_gather_results as well -- its N > 1 branch executed on a one-GPU box (test mode; real RCCL refuses two ranks on a device)
    loopback = bool(os.environ.get("PR_RCCL_LIBRARY")) and threads_mode and share_device
    gather_mode = "host" if ((share_device and not loopback) or want == "host") else ("torch" if (want == "torch" and not threads_mode) else "cabi")
    gather_note = comm_note
    if multi and gather_mode == "cabi" and threads_mode and not comm_ready and not loopback:
        gather_mode = "host"
    if multi and gather_mode == "cabi" and (not threads_mode or loopback):
        try:
            ident = group.all_gather(api.comm_id() if rank == 0 else None)[0]    # 128 bytes, once
            api.comm_init_rank(ident, rank, world)
        except Exception as e:                                     # noqa: BLE001 -- a failed bootstrap must not cost the measurement
            print(f"[bench] rank {rank}: C-ABI communicator unavailable ({e}); falling back to {'host copies' if threads_mode else 'torch.distributed.gather'}", file=sys.stderr, flush=True)
            gather_mode = "host" if threads_mode else "torch"
            gather_note = f"C-ABI bootstrap failed on rank {rank}: {e}"
        notes = group.all_gather(gather_note)
        if any(notes):                                             # one rank without a communicator: every rank uses torch's gather, and the line says why
            gather_mode = "host" if threads_mode else "torch"
            gather_note = "; ".join(n for n in notes if n)
    if multi:
        group.barrier()                                             # every rank's communicators exist (and have printed what they print)
    flush_c_stdio()
    api.set_option("blocking_wait", (1 if world > 1 else 0) if args.blocking_wait < 0 else args.blocking_wait)
    api.set_option("solve", api.SOLVE_DEVICE if args.solve == "device" else api.SOLVE_HOST)
    api.set_option("pose_groups", args.pose_groups)
    api.set_option("fused_solve", args.fused_solve)
    if args.overlap_pass >= 0:
        api.set_option("overlap_pass", args.overlap_pass)
    for kv in args.opt:
        name, value = kv.split("=")
        api.set_option(name, int(value))

    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    scene_depth = api.render_host(model, synth.scene_pose()[None], W, H, proj)[0]
    scene = (api.Scene_projective().init_Scene_projective_cuda(scene_depth, K) if args.scene == "proj"
             else api.Scene_nn().init_Scene_nn_cuda(scene_depth, K))
    crit = api.ICPConvergenceCriteria(0.0, 0.0, args.iters)
    sample_profile = int(os.environ.get("PR_BENCH_SAMPLE_PROFILE", "3"))

    class Job:
        """K steps of one global batch size: this rank's contiguous shard [first, first + P) of the seeded hypothesis stream
        (prd.shard_bounds == pr_shard_range of the C ABI), refined through the two asynchronous slots -- step k is SUBMITTED on slot k & 1
        (everything enqueued, no host round trip) and only then is step k-1 waited for -- with the results of step k going to record
        block k of one device buffer.  The gather: ONE exchange of all K x P records after the last step (`job`), or one per step enqueued
        behind its batch and overlapped with the next (`step`)."""

        def __init__(self, global_poses, steps, gather_when):
            self.global_poses, self.steps = global_poses, max(1, steps)
            self.first, self.P = prd.shard_bounds(global_poses, rank, world)
            self.P_max = prd.shard_bounds(global_poses, 0, world)[1]
            if self.P == 0:
                raise SystemExit(f"rank {rank}: empty shard ({global_poses} hypotheses over {world} ranks)")
            self.poses = synth.hypotheses(self.P, seed=6, first=self.first)
            self.gather_when = gather_when
            self.gather_why = None
            if multi and gather_when == "job" and global_poses % world != 0:
                # the K x P blocks of uneven shards are not the shards of K x global records: exchange per step instead
                self.gather_when, self.gather_why = "step", f"{global_poses} hypotheses do not divide over {world} ranks evenly: one exchange per step"
            self.res = api.DeviceVector(self.steps * self.P * 18, np.float32)           # K blocks of P x RegistrationResult (72 B)
            n_recv = self.steps * global_poses if self.gather_when == "job" else 2 * global_poses
            self.recv = api.DeviceVector(n_recv * 18, np.float32) if (multi and rank == 0 and gather_mode == "cabi") else None
            self.inflight = [None, None]                              # slot -> step index submitted, not yet waited for
            self.k = 0
            self.last_sizes = self.last_results = None
            self.gathers = 0
            self.host_gathered = None

        def block(self, k):
            return self.res.data() + (k % self.steps) * self.P * 72

        def exchange(self, send_ptr, n_local, n_total, recv_slot=0):
            """One gather of n_local records per rank to rank 0."""
            self.gathers += 1
            if gather_mode == "cabi":
                api.gather_results(send_ptr, n_local, n_total, 0, (self.recv.data() + recv_slot * n_total * 72) if rank == 0 else None)
            elif gather_mode == "torch":
                import torch
                api.sync()
                t = torch.empty(n_local * 18, dtype=torch.float32, device="cuda")
                api._lib.check(api._lib.load().pr_memcpy_d2d(t.data_ptr(), send_ptr, n_local * 72))
                prd.gather_results(t, world, rank, dst=0, max_count=max(prd.shard_bounds(n_total, r, world)[1] for r in range(world)))
            else:                                                    # ranks share one device (test mode): host copies through the control plane
                api.sync()
                h = np.empty(n_local * 18, np.float32)
                api._lib.check(api._lib.load().pr_memcpy_d2h(api.ptr(h), send_ptr, h.nbytes))
                parts = group.all_gather(h)
                if rank == 0:
                    self.host_gathered = np.concatenate(parts)

        def retire(self, b):
            k = self.inflight[b]
            if k is None:
                return
            res, sizes = api.refine_wait(b)
            self.inflight[b] = None
            self.last_sizes, self.last_results = sizes, res
            if multi and self.gather_when == "step":              # enqueued on the library's stream behind this batch (cabi), under the next step
                self.exchange(self.block(k), self.P, self.global_poses, recv_slot=k & 1)

        def step(self):
            b = self.k & 1
            # the 72-byte records go to the job's device block (what a sharded job's gather reads) AND to the host, like the reference's by-value
            # RegistrationResult (icp.cu:156-223): SURVEY 8d counts the result D2H inside the metric (VERDICT r05 missing 5)
            api.refine_submit(b, model, self.poses, W, H, proj, K, scene, crit, results_dev=self.block(self.k), also_host=True)
            self.inflight[b] = self.k
            self.k += 1
            self.retire(1 - b)

        def fence(self, gather=True):
            for b in (0, 1):
                self.retire(b)
            if multi and gather and self.gather_when == "job":  # the job's single exchange: every record of the K steps, 72 B each
                self.exchange(self.res.data(), self.steps * self.P, self.steps * self.global_poses)
            api.sync()                                           # the library stream carries the batches and the gathers
            if multi:
                group.barrier()

        def sample(self):
            """One step with HIP events around every correspondence launch, its loop alone on the chip (option profile = 3)."""
            sync = group.barrier if (threads_mode and multi) else (lambda: None)   # library options are process-wide: rank THREADS switch them at the same point
            sync()
            api.set_option("profile", sample_profile)
            sync()
            self.step()
            self.fence(gather=False)
            api.set_option("profile", 0)
            sync()

        def run(self, warmup, burn_in=0, sample_in="warmup", sequential=False, marks_out=None):
            """`warmup` untimed steps, then exactly `steps` timed ones between two fences (barrier + device drained on both sides).
            Returns (elapsed seconds, profile of the sampled launches or None, launch durations of the sample)."""
            prof, launches_us = None, None
            for _ in range(max(0, burn_in)):
                self.step()
            if not sequential:
                api.profile_reset()
            for w in range(warmup):
                # the first warm-up step is a timed one: a slot creates its HIP events (46 of them, several microseconds each) on first use, and
                # that belongs to the warm-up like every other first use.  The LAST warm-up step is the roofline sample (--sample-in warmup).
                if sequential or sample_in is None:
                    self.step()
                elif w == warmup - 1 and sample_in == "warmup":
                    self.fence(gather=False)
                    api.profile_reset()
                    self.sample()
                    prof, launches_us = api.profile_read(), api.profile_launches()
                elif w == 0:
                    self.sample()
                else:
                    self.step()
            api.set_option("profile", 1 if sequential else 0)
            if sequential or prof is None:
                api.profile_reset()
            self.fence()                                             # also warms the job's exchange up
            self.k = 0
            self.gathers = 0
            c0 = time.process_time()
            t0 = time.perf_counter()
            for i in range(self.steps):
                if prof is None and sample_in in ("timed", "warmup") and not sequential and i == self.steps - 1:
                    api.set_option("profile", sample_profile)        # --sample-in timed (or no warm-up step to sample): the last timed step
                self.step()
                if marks_out is not None:
                    marks_out.append(time.perf_counter() - t0)
            self.fence()
            elapsed = time.perf_counter() - t0
            self.cpu_timed_s = time.process_time() - c0                # CPU seconds of every thread of this process over the TIMED region only
            self.gathers_timed = self.gathers                        # exchanges inside the timed region (the sample step below is outside it)
            self.timed_results, self.timed_sizes = self.last_results, self.last_sizes      # what the last timed step returned (--dump-outputs)
            api.set_option("profile", 0)
            if sequential:
                prof, launches_us = api.profile_read(), api.profile_launches()
                self.sampled_in = "every step (--sequential)"
            elif sample_in is None:                                  # no roofline sample asked for (a plain run)
                self.sampled_in = None
            elif sample_in == "after":
                api.profile_reset()
                self.sample()                                        # one more step, untimed: same batch, same kernels and arguments as every timed step
                prof, launches_us = api.profile_read(), api.profile_launches()
                self.sampled_in = "after (one untimed step behind the timed region's closing fence)"
            elif prof is None:
                prof, launches_us = api.profile_read(), api.profile_launches()
                self.sampled_in = "timed region (its last step)"
            else:
                self.sampled_in = "warmup (the last warm-up step)"
            return elapsed, prof, launches_us

    def over_ranks(elapsed, steps):
        """max over ranks of the elapsed time, and every rank's own ms per step"""
        mine = 1e3 * elapsed / steps
        if not multi:
            return elapsed, [mine]
        both = group.all_gather((elapsed, mine))
        return max(e for e, _ in both), [m for _, m in both]

    def cpu_over_ranks(cpu_s, wall_s, steps):
        """every rank's host CPU time over its timed region: ms per step and CPU-seconds per wall-second.  One process per rank: the
        process' own clock (all its threads: the caller, the library's helper threads, the HIP runtime's).  Host threads as ranks share
        one process clock: the total is reported once and divided by the ranks."""
        if not multi:
            return [1e3 * cpu_s / steps], [cpu_s / wall_s if wall_s > 0 else None]
        if threads_mode:
            both = group.all_gather((cpu_s / world, wall_s))
        else:
            both = group.all_gather((cpu_s, wall_s))
        return [1e3 * c / steps for c, _ in both], [(c / w if w > 0 else None) for c, w in both]

    if args.scaling == "strong":
        global_poses = args.global_poses or 4096
    else:
        global_poses = args.global_poses or args.poses * world
    job = Job(global_poses, args.steps, args.gather)
    P, P_max = job.P, job.P_max
    cpu0 = time.process_time()
    marks = []
    # Roofline sample: ONE step with profile 3 -- an asynchronous batch like every other (its render runs under the previous step's loop, no
    # host round trip), but its loop runs as one pose group, starts when the other slot's batch is complete and carries HIP events around
    # every correspondence launch, so the timed launches have the chip to themselves.  By default it is ONE MORE STEP BEHIND the timed region's
    # closing fence: the same batch, the same kernels and arguments as every timed step, without its exclusive loop (which overlaps with
    # nothing: ~0.5 ms) counting against `value` -- a 20-step region is 21 ms -- and on a device that has been under load for the whole run
    # (sampled in the last warm-up step, 5 ms after the first launch, the same launches read 41.9 instead of 39.2 us: clocks still coming up).
    # --sample-in timed puts it back into the timed region (its last step, as in rounds 1-3), --sample-in warmup into the last warm-up step.
    # Only --full (or an explicit --sample-in) takes the sample: a plain run has no `roofline`.
    sample_in = args.sample_in or ("after" if args.full else None)
    elapsed, prof, launches_us = job.run(args.warmup, burn_in=args.burn_in, sample_in=sample_in, sequential=args.sequential, marks_out=marks)
    step_ms = np.diff(np.asarray([0.0] + marks)) * 1e3               # host clock after every step's (submit + wait for the step before it); the closing fence comes on top
    if os.environ.get("PR_BENCH_MARKS") and rank == 0:             # where a run's time went: cumulative ms after every step's submit + previous wait, and the closing fence
        print("[bench] marks ms:", " ".join(f"{1e3 * m:.2f}" for m in marks), "| fence", f"{1e3 * (elapsed - marks[-1]):.2f}", file=sys.stderr, flush=True)
    wall_s_rank0 = elapsed                                           # this rank's own clock (before the max over ranks)
    host_cpu_s = job.cpu_timed_s                                     # CPU time of ALL threads of this process over the timed region (round 5: warm-up excluded)
    wall_s = elapsed
    rank_cpu_ms, rank_cpu_per_wall = cpu_over_ranks(host_cpu_s, wall_s, args.steps)
    sizes = job.timed_sizes
    gathers_timed = job.gathers_timed
    gather_ms, gather_n = (api.gather_profile() if (multi and gather_mode == "cabi") else (0.0, 0))
    elapsed, per_rank_ms = over_ranks(elapsed, args.steps)

    # BASELINE configs[3] next to the weak-scaling line: 4096 hypotheses per step over the N ranks (512 per GPU on 8), same loop, same gather
    config3 = None
    if args.full and multi and world > 1 and not args.no_config3 and args.scene == "proj" and not args.sequential and global_poses != 4096:
        k3 = min(args.steps, 20)
        job3 = Job(4096, k3, args.gather)
        e3, _, _ = job3.run(min(args.warmup, 3), sample_in=None)
        e3, per3 = over_ranks(e3, k3)
        config3 = {"workload": f"BASELINE configs[3]: obj_06.ply, 4096 hypotheses per step sharded over {world} GPUs ({job3.P_max} per GPU), projective, {args.iters} ICP iterations, "
                               f"{'ONE gather of all ' + str(k3) + ' x 4096 records' if job3.gather_when == 'job' else 'one gather per step'}",
                   "value": 4096 * k3 / e3, "unit": "poses/s", "ms_per_step": 1e3 * e3 / k3, "steps": k3, "scaling": "strong", "global_batch": 4096,
                   "poses_per_gpu": job3.P_max, "per_rank_ms_per_step": per3, "gathers": job3.gathers_timed}

    flush_c_stdio()
    if multi:
        group.barrier()                                             # nothing of any rank is left to be written before rank 0's line
    if rank != 0:
        return None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, job.timed_results, job.timed_sizes)

    total_poses = global_poses * args.steps
    n_mean = float(np.mean(sizes))
    out = {
        "metric": "refined poses/sec (640x480, 20 ICP iters)",
        "value": total_poses / elapsed,
        "unit": "poses/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "burn_in_steps": max(0, args.burn_in),                   # untimed, before the warm-up steps: device clocks up from idle
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"obj_06.ply, {P_max}-pose batch per GPU, 640x480 synthetic depth, "
                               f"{'projective' if args.scene == 'proj' else 'kd-tree NN (exact search with the reference tie-breaks: keep-the-winner test and pixel-window scan where the bound allows, order-free task walk over 128-byte wide nodes otherwise, ties repeated by the ordered walk)'} association, "
                               f"{args.iters} ICP iterations (21 passes), solve on {args.solve}"
                               + (f", {args.pose_groups or 2} pose groups" if args.solve == "device" else ""),
                   "poses_per_gpu": P_max, "global_batch": global_poses, "points_per_pose_mean": float(np.mean(sizes)),
                   "parallelism": (f"pose-shard x{world}, no data-path collective, "
                                   + ("no gather (1 rank)" if not multi else
                                      (f"{'ONE gather of the job (all K x P records after the last step)' if job.gather_when == 'job' else '1 gather per step'}: "
                                       + {"cabi": "pr_gather_results (RCCL)", "torch": "torch.distributed.gather (RCCL backend)",
                                          "host": "host copies through the control plane (ranks share one device: test mode)"}[gather_mode])))},
        "launcher": {"kind": group.kind,
                     "how": (os.environ.get("PR_BENCH_LAUNCHED_BY") or
                             {"solo": "one process, one GPU", "threads": "one process, one host thread per GPU (pr_comm_init_all + pr_set_device per thread)",
                              "processes": "one process per GPU, started by the caller's launcher (torch.distributed.run / torchrun environment)"}[group.kind]),
                     "note": launcher_note, "share_device_test_mode": share_device},
        "gather": ("none (1 rank)" if not multi else {"cabi": "pr_gather_results: grouped ncclSend/ncclRecv on the library stream (C ABI over " + ("the loop-back stand-in PR_RCCL_LIBRARY: test mode)" if os.environ.get("PR_RCCL_LIBRARY") else "RCCL)"),
                                                        "torch": "torch.distributed.gather (RCCL)",
                                                        "host": "host copies through the control plane (ranks share one device: test mode)"}[gather_mode]),
        "gather_when": (job.gather_when if multi else None), "gather_when_note": job.gather_why, "gathers_in_timed_region": gathers_timed if multi else 0,
        "gather_bytes_per_rank": (72 * P * (args.steps if job.gather_when == "job" else 1)) if multi else 0,
        "gather_note": gather_note,
        "gather_event_us": (1e3 * gather_ms / gather_n) if gather_n else None,      # HIP events around the exchange on the library stream, sampled steps (rank 0)
        "gather_events": int(gather_n),
        "per_rank_ms_per_step": per_rank_ms,
        "host_cpu_per_wall": host_cpu_s / wall_s if wall_s > 0 else None,   # rank 0's process: CPU seconds (all threads) per second, both over the timed region only
        "host_cpu_ms_per_step": 1e3 * host_cpu_s / args.steps,
        "per_rank_host_cpu_ms_per_step": rank_cpu_ms, "per_rank_host_cpu_per_wall": rank_cpu_per_wall,
        "host_cpu_note": ("one process, host threads as ranks: the process' CPU time divided by the ranks" if threads_mode else "per rank: the process' CPU time (all its threads) over its timed region"),
        # the timed steps one by one (host clock between consecutive submits of the pipelined loop; the first two fill the pipeline), and the closing fence
        "step_ms_spread": ({"min": float(step_ms.min()), "median": float(np.median(step_ms)), "max": float(step_ms.max()), "n": int(len(step_ms)),
                            "steady_median": float(np.median(step_ms[2:])) if len(step_ms) > 4 else None,
                            "closing_fence_ms": float(1e3 * wall_s_rank0 - 1e3 * marks[-1])} if len(step_ms) else None),
        "blocking_wait": bool(api.get_option("blocking_wait")),
    }
    if prof is not None:                                             # the roofline sample was taken (--full, --sample-in or --sequential)
        launches = max(1, prof["icp_launches"])
        pts_per_launch = prof["icp_points"] / launches
        bytes_per_launch = prof["icp_bytes"] / launches          # 36 B/point on pass 0, 48 B/point afterwards
        avg_launch_s = prof["icp_kernel_ms"] * 1e-3 / launches
        achieved = bytes_per_launch / avg_launch_s if avg_launch_s > 0 else 0.0
        traffic = PMC_TRAFFIC_BYTES_PER_POINT[args.scene] * pts_per_launch if PMC_TRAFFIC_BYTES_PER_POINT[args.scene] else None
        traffic_source = ("committed rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE passes, "
                          + PMC_TRAFFIC_SOURCE[args.scene] + f": {PMC_TRAFFIC_BYTES_PER_POINT[args.scene]} B/point x points of a launch")
        live = dram = None
        if args.full and world == 1 and not multi and not args.no_live_pmc and not args.sequential:
            live = live_pmc_traffic(args.scene)                     # two counter passes of the same kernels, run now
            if args.scene == "proj":
                dram = live_pmc_traffic("proj", n_poses=1024, opts="sub_batch=1024,pose_groups=1", with_duration=True)
        if live:
            traffic = live["bytes_per_point"] * pts_per_launch
            traffic_source = live["source"]
        # what DRAM really carries: 1024 hypotheses as ONE sub-batch (270 MB of clouds: more than the 256 MiB Infinity Cache holds)
        if dram and dram.get("launch_us"):
            frac_dram = dram["bytes_per_point"] * dram["points_per_dispatch"] / (dram["launch_us"] * 1e-6) / HBM_PEAK
            dram_note = (f"this run: 1024 hypotheses as one sub-batch (clouds exceed the Infinity Cache), {dram['bytes_per_point']:.1f} B/point x {dram['points_per_dispatch']} points "
                         f"per {dram['launch_us']:.1f} us launch (rocprofv3 --kernel-trace pass of the same workload)")
        else:
            frac_dram, dram_note = PMC_DRAM_FRAC.get(args.scene), PMC_DRAM_SOURCE
        lus = np.sort(np.asarray(launches_us, np.float64)) if launches_us is not None and len(launches_us) else None
        valu_rate = (PMC_VALU_WAVE_INSTR_PER_POINT[args.scene] * pts_per_launch / avg_launch_s) if (PMC_VALU_WAVE_INSTR_PER_POINT[args.scene] and avg_launch_s > 0) else None
        # SURVEY 8d, per hypothesis: render 36 T + 4 W H (clear) + 4 W H (read by the extraction) = 3.59 MB; cloud 12 N; loop: projective
        # N (21 x 36 + 20 x 12) = 996 N, kd-tree (HBM-compulsory) N (21 x 12 + 20 x 12) = 492 N
        e2e_bytes_per_pose = (36.0 * len(model.tris) + 8.0 * W * H) + 12.0 * n_mean + (996.0 if args.scene == "proj" else 492.0) * n_mean
        n_samples = 1
        valu_frac = (valu_rate / VALU_PEAK) if valu_rate else None
        profiled_ok = pmc_constants_current()
        if args.scene == "proj":
            verdict = ("valu" if (valu_frac or 0) >= 0.6 else ("dram" if (frac_dram or 0) >= 0.6 else "latency"))
            binding = {"verdict": verdict,
                       "rule": "valu if VALU issue >= 0.6 of the calibrated peak, dram if the DRAM counter figure >= 0.6 of 8 TB/s, else latency",
                       "valu_issue_frac": valu_frac, "valu_wave_instr_per_s": valu_rate, "valu_peak_wave_instr_per_s": VALU_PEAK, "valu_peak_source": VALU_PEAK_SOURCE,
                       "valu_wave_instr_per_point": PMC_VALU_WAVE_INSTR_PER_POINT[args.scene],
                       "valu_wave_instr_per_point_source": "COMMITTED constant, not a counter of this run: " + PMC_TRAFFIC_SOURCE[args.scene].split(" + sq_")[0].split("pmc_")[0]
                                                           + "sq_proj_SQ_INSTS_VALU_SQ_INSTS_VMEM_SQ_INSTS_LDS.md; the kernel's sources "
                                                           + ("are unchanged since that pass" if profiled_ok else "HAVE CHANGED since that pass: the figure is stale until the SQ pass is repeated"),
                       "valu_constants_stale": (not profiled_ok),
                       "dram_frac_counter": frac_dram, "dram_frac_counter_source": dram_note,
                       "wait_frac": PROJ_PASS_WAIT_FRAC, "wait_frac_source": "committed: profiles/r06/sq_proj_SQ_ACTIVE_INST_VALU_SQ_WAVE_CYCLES_SQ_WAIT_INST_ANY.md, SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES of icp_pass_kernel<SceneProjPacked> (1.07e9 of 3.48e9)",
                       "note": "a lane keeps four scene gathers in flight; 16 wavefronts per CU; the kernel saturates neither VALU issue nor DRAM"}
        else:
            binding = {"verdict": "latency (cache-resident search: HBM carries only clouds and winners)", "valu_issue_frac_walk_pass0": NN_WALK_VALU_ISSUE_FRAC,
                       "valu_peak_wave_instr_per_s": VALU_PEAK, "valu_peak_source": VALU_PEAK_SOURCE}
        out.update({
            # The contract's block: `bound` names the roof SURVEY 8d prices this kernel against (HBM), `achieved` = 8d's ALGORITHMIC bytes of the sampled
            # launches over their HIP-event time, `peak` = 8 TB/s, `frac` = achieved / peak, `traffic` = the PMC bytes of one launch.  (Round 5 put the VALU
            # issue share into `frac`, against a peak that round 6's calibration showed to be 1.6x too low: VERDICT r05 weak 5.)  What the counters say really
            # limits the kernel is in `binding`: VALU issue against the CALIBRATED peak, DRAM by counter for a batch that spills the Infinity Cache, and the
            # share of wave-cycles spent waiting -- with none of the units at 0.6 the verdict is "latency".
            "roofline": {"bound": "hbm",
                         "kernel": ("icp_pass_kernel (correspondence + 29-term reduce" if args.scene == "proj" else
                                                     "one correspondence pass = nn_search_kernel + nn_bound_kernel + nn_tree_wide_kernel + icp_pass_kernel<SceneNNWinners> (search, bound + window, task walk of the queued queries, 29-term reduce over the winners")
                                                    + (" + finalize/solve tail)" if args.fused_solve and args.solve == "device" else ")"),
                         "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": achieved / HBM_PEAK,
                         "frac_of": "HBM peak (8 TB/s), SURVEY 8d algorithmic bytes: 36 B/point on the first and last pass, 48 B/point between",
                         "frac_algorithmic": achieved / HBM_PEAK,
                         "binding": binding,
                         "frac_end_to_end": e2e_bytes_per_pose * (total_poses / elapsed) / HBM_PEAK,
                         "end_to_end_algorithmic_bytes_per_pose": e2e_bytes_per_pose,
                         "frac_fabric_counter": (traffic / avg_launch_s / HBM_PEAK) if (traffic and avg_launch_s > 0) else None,
                         "frac_dram_counter": frac_dram, "frac_dram_counter_source": dram_note, "dram_live": dram,
                         "traffic": traffic,
                         "traffic_source": traffic_source,
                         "traffic_live": live,
                         "residency": "clouds of a sub-batch (<= 512 hypotheses) stay in the 256 MiB Infinity Cache over the 21 passes; scene records are L2-resident",
                         "avg_launch_us": avg_launch_s * 1e6, "launches": int(launches),
                         # the sampled launches one by one: pass 0 and the score-only last pass move 36 B/point, the others 48
                         "launch_us_spread": ({"min": float(lus[0]), "median": float(np.median(lus)), "max": float(lus[-1]), "n": int(len(lus))} if lus is not None else None),
                         "algorithmic_bytes_per_launch": bytes_per_launch, "points_per_launch": pts_per_launch,
                         "sampled_in": job.sampled_in,
                         "share_device_note": ("ranks share ONE device (test mode): the sampled launches run beside the other ranks' work, so avg_launch_us / frac of this line say nothing about the kernel" if share_device else None),
                         "timing": ("HIP events on the library stream around every launch (--sequential: synchronous single-group steps)" if args.sequential else
                                    f"HIP events on the library stream around every launch of {n_samples} step ({job.sampled_in}); "
                                    "the sampled step stays an asynchronous batch but its loop runs as one pose group and only once the other slot's batch is complete (option profile = 3), so the launch has the chip to itself")},
            "phase_ms_per_timed_step": {"render": prof["render_ms"] / max(1, launches // (args.iters + 1)),
                                        "cloud": prof["cloud_ms"] / max(1, launches // (args.iters + 1))},
        })
    if config3:
        out["config3_4096_global"] = config3
    solo = args.full and world == 1 and not multi                  # the other configurations and the CPU baseline: --full only
    if solo and args.scene == "proj" and args.solve == "device" and not args.sequential and not args.no_kdtree_extra:
        out["solve_on_host"] = host_solve_extra(args, api, model, job.poses, W, H, proj, K, scene)
    if "solve_on_host" in out:
        # `north_star` words the solve as "SVD solve on host": that configuration's figure next to the headline's, in `config` (the full record: `solve_on_host`)
        out["config"]["north_star_solve_on_host"] = {"value": out["solve_on_host"]["value"], "unit": "poses/s", "ms_per_step": out["solve_on_host"]["ms_per_step"],
                                                     "one_synchronous_call_per_step": out["solve_on_host"]["one_synchronous_call_per_step"]["value"],
                                                     "note": "same batches, PR_SOLVE_HOST, pipelined through the two slots from one caller thread; the headline `value` keeps the 6x6 solve on the device"}
    if solo and args.scene == "proj" and not args.no_kdtree_extra and not args.sequential:
        out["config2_kdtree"] = kdtree_extra(args, api, model, job.poses, scene_depth, W, H, proj, K)
    if solo and not args.no_kdtree_extra and not args.sequential:
        out["default_criteria"] = default_criteria_extra(args, api, model, job.poses, scene_depth, W, H, proj, K)
    if solo and not args.no_kdtree_extra and not args.sequential:
        out["new_scene_per_frame"] = new_scene_extra(args, api, model, job.poses, scene_depth, W, H, proj, K)
    if solo and args.scene == "proj" and args.solve == "device" and not args.no_kdtree_extra and not args.sequential:
        # BASELINE configs[3] and configs[4] as ONE GPU sees them (its share of the sharded job), so that a single-GPU run records them too
        out["config3_share_512"] = share_extra(api, "config3", "BASELINE configs[3], one GPU's share: obj_06.ply, 512 of the 4096 hypotheses (rank 0's contiguous shard), 640x480, projective, "
                                               f"{args.iters} ICP iterations, two asynchronous slots", model, synth.hypotheses(512), W, H, proj, K, scene, args.iters, 20, len(model.tris),
                                               "the N > 1 line carries the sharded job itself (config3_4096_global)")
        W5, H5, K5 = 1280, 720, synth.intrinsics_720p()
        tris5 = synth.uv_sphere_mesh()
        model5 = api.Model(tris=tris5)
        proj5 = api.compute_proj(K5, W5, H5)
        sd5 = api.render_host(model5, synth.scene_pose()[None], W5, H5, proj5)[0]
        scene5 = api.Scene_projective().init_Scene_projective_cuda(sd5, K5, W5, H5)
        out["config4_share_128"] = share_extra(api, "config4", "BASELINE configs[4], one GPU's share: 1 000 000-triangle synthetic mesh (SURVEY 8d's UV sphere), 1280x720 depth render + projective ICP, "
                                               f"128 of the 1024 hypotheses, {args.iters} ICP iterations, two asynchronous slots", model5, synth.hypotheses(128), W5, H5, proj5, K5, scene5,
                                               args.iters, 12, len(tris5), "parity: tests/test_configs_gpu.py (render bit-exact, two hypotheses against the oracle) and tests/golden/config4.npz (all 128)")
        del scene5, model5
    if solo and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, args.scene, model.tris, scene_depth, K, W, H)
        if "config2_kdtree" in out:
            out["config2_kdtree"]["cpu_baseline"] = cpu_baseline(args, "nn", model.tris, scene_depth, K, W, H)
    return out


def dump_outputs(out_dir, results, sizes):
    """What the last timed step returned to its caller: the RegistrationResult records (T row-major, fitness, inlier_rmse: float32)
    and the cloud sizes (float64: exact for uint32) as out_dir/<name>.npy -- 80 bytes per hypothesis."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"T": results["T"], "fitness": results["fitness"], "inlier_rmse": results["inlier_rmse"], "sizes": sizes.astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


# sha256 (first 16 hex digits) of the sources of icp_pass_kernel<SceneProjPacked> at the time the committed SQ / PMC constants above were measured:
# when the kernel's sources change, the line says that the VALU figures are stale instead of presenting them as measured
PMC_PROFILED_SOURCES = ("icp_pass.hip", "icp_accumulate.h", "proj_query.h", "icp_solve_device.h", "pr_tuning.h")
PMC_PROFILED_HASH = "d39e369ab211c4d6"


def pmc_sources_hash():
    import hashlib
    h = hashlib.sha256()
    for name in PMC_PROFILED_SOURCES:
        with open(os.path.join(ROOT, "pose_refine_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def pmc_constants_current():
    try:
        return pmc_sources_hash() == PMC_PROFILED_HASH
    except OSError:
        return False


def share_extra(api, label, workload, model, poses, W, H, proj, K, scene, iters, steps, n_tris, note):
    """One more BASELINE workload in the N = 1 line (VERDICT r05 missing 4): the per-GPU SHARE of a sharded configuration, pipelined through the two
    slots like the headline (records to the host inside the timed region), with SURVEY 8d's end-to-end fraction of the HBM roof."""
    import numpy as np
    crit = api.ICPConvergenceCriteria(0.0, 0.0, iters)
    sizes = None
    for k in range(3):
        api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
        if k:
            api.refine_wait((k - 1) & 1)
    api.refine_wait(0)
    seg = []
    for _ in range(3):                                           # three segments, the median is the figure (see host_solve_extra)
        t0 = time.perf_counter()
        for k in range(steps):
            api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
            if k:
                _, sizes = api.refine_wait((k - 1) & 1)
        res, sizes = api.refine_wait((steps - 1) & 1)
        seg.append((time.perf_counter() - t0) / steps)
    dt = sorted(seg)[1]
    n_mean = float(np.mean(sizes))
    bytes_per_pose = 36.0 * n_tris + 8.0 * W * H + 12.0 * n_mean + 996.0 * n_mean          # render + cloud + projective loop
    value = len(poses) / dt
    return {"workload": workload, "value": value, "unit": "poses/s", "ms_per_step": 1e3 * dt, "steps": steps, "poses_per_gpu": int(len(poses)),
            "segments_poses_per_s": [len(poses) / d for d in seg], "value_is": "the median of three consecutive segments of `steps` pipelined steps",
            "points_per_pose_mean": n_mean, "mean_fitness": float(np.mean(res["fitness"])),
            "end_to_end_algorithmic_bytes_per_pose": bytes_per_pose, "hbm_ceiling_poses_per_s": HBM_PEAK / bytes_per_pose,
            "frac_end_to_end": bytes_per_pose * value / HBM_PEAK, "note": note}


def live_pmc_traffic(scene_kind, n_poses=256, opts="pose_groups=1", with_duration=False):
    """(with_duration: a third child pass, `--kernel-trace` alone, gives the same kernels' average launch time for the same workload.)
    roofline.traffic measured by this run: two `rocprofv3 --kernel-trace --pmc <counter>` passes (FETCH_SIZE, WRITE_SIZE: one counter per
    pass, as MI355X_MICROARCH.md prescribes) of tools/pmc_workload.py -- three 256-hypothesis batches of the same workload as ONE pose group, so
    that a dispatch covers every cloud of the batch -- in child processes, read back from the rocpd databases.  FETCH_SIZE is corrected by
    the factor this very pass shows on max2zero_kernel, which reads and writes a known number of bytes (2.0 on gfx950; outside 1.8-2.2 the
    guide's 2 is used; WRITE_SIZE likewise: 1.0).  Returns None when anything is missing or fails: the line then carries the committed figures."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    kernels = (["icp_pass_kernel<prk::SceneProjPacked"] if scene_kind == "proj" else
               ["nn_search_kernel", "nn_bound_kernel", "nn_tree_wide_kernel", "icp_pass_kernel<prk::SceneNNWinners"])
    try:
        per_dispatch = {}                                          # counter -> KB per dispatch, summed over the kernels of a pass
        calib = {}
        points = None
        with tempfile.TemporaryDirectory(dir="/tmp") as d:
            env = dict(os.environ, TMPDIR="/tmp", PR_OPTS=opts, PR_RASTER_MODE="0")
            launch_us = None
            if with_duration:
                cmd = [exe, "--kernel-trace", "-d", d, "-o", "trace", "--", sys.executable, os.path.join(ROOT, "tools", "pmc_workload.py"), str(n_poses)] + ([] if scene_kind == "proj" else ["nn"])
                r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=120)
                dbs = glob.glob(os.path.join(d, "**", "trace_results.db"), recursive=True)
                if r.returncode == 0 and dbs:
                    con = sqlite3.connect(dbs[0])
                    rows = list(con.execute("select name, (end - start) / 1000.0 from kernels"))
                    con.close()
                    tot = 0.0
                    for k in kernels:
                        v = [us for n, us in rows if k in n]
                        if not v:
                            tot = None
                            break
                        tot += sum(v) / len(v)
                    launch_us = tot
            for counter in ("FETCH_SIZE", "WRITE_SIZE"):
                cmd = [exe, "--kernel-trace", "--pmc", counter, "-d", d, "-o", counter, "--", sys.executable, os.path.join(ROOT, "tools", "pmc_workload.py"), str(n_poses)]
                if scene_kind != "proj":
                    cmd.append("nn")
                r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=120)
                for line in r.stdout.splitlines():
                    if line.startswith("points per batch:"):
                        points = int(line.split(":")[1])
                dbs = glob.glob(os.path.join(d, "**", counter + "_results.db"), recursive=True)
                if r.returncode != 0 or not dbs or not points:
                    return None
                con = sqlite3.connect(dbs[0])
                rows = list(con.execute("select name, count(*), sum(counter_value) from pmc_events where counter_name = ? group by name", (counter,)))
                con.close()
                total = 0.0
                for k in kernels:
                    hit = [(n, c, v) for n, c, v in rows if k in n]
                    if not hit:
                        return None
                    total += sum(v for _, _, v in hit) / sum(c for _, c, _ in hit)
                per_dispatch[counter] = total
                # calibration: the workload's two max2zero launches (one scene image, then the n_poses images of a public render call) read
                # and write every pixel of n_poses + 1 images of 640 x 480 int32 -- known bytes against the counter's sum over both
                cal = [v for n, c, v in rows if "max2zero_kernel" in n]
                if cal and cal[0] > 0:
                    calib[counter] = ((n_poses + 1) * 640 * 480 * 4 / 1024.0) / cal[0]
        f_fetch = calib.get("FETCH_SIZE", 2.0)
        if not (1.8 <= f_fetch <= 2.2):
            f_fetch = 2.0
        f_write = calib.get("WRITE_SIZE", 1.0)
        if not (0.9 <= f_write <= 1.1):
            f_write = 1.0
        kb = f_fetch * per_dispatch["FETCH_SIZE"] + f_write * per_dispatch["WRITE_SIZE"]
        bpp = kb * 1024.0 / points
        return {"bytes_per_point": bpp, "fetch_kb_per_dispatch": per_dispatch["FETCH_SIZE"], "write_kb_per_dispatch": per_dispatch["WRITE_SIZE"],
                "fetch_correction": f_fetch, "write_correction": f_write, "points_per_dispatch": points, "launch_us": launch_us, "hypotheses": n_poses, "options": opts,
                "source": (f"this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (one pass each) of tools/pmc_workload.py {n_poses} ({opts}) -- "
                           f"({f_fetch:.3f} x {per_dispatch['FETCH_SIZE']:.0f} + {f_write:.3f} x {per_dispatch['WRITE_SIZE']:.0f}) KB per dispatch of {points} points = {bpp:.1f} B/point "
                           f"(fabric side: Infinity-Cache hits included), x points of a launch; both counters corrected by what max2zero_kernel (known bytes) shows in the same pass")}
    except Exception as e:                                         # noqa: BLE001 -- an extra: never at the cost of the line
        print(f"[bench] live PMC pass unavailable ({e}); the line carries the committed counter figures", file=sys.stderr, flush=True)
        return None


def kdtree_extra(args, api, model, poses, scene_depth, W, H, proj, K, steps=20):
    """BASELINE.json configs[2] next to the headline: the same 256-hypothesis batch against the kd-tree scene (Scene_nn), a
    few steps through the two asynchronous slots, plus one instrumented (synchronous) batch whose work counters give the LOGICAL bytes of the
    search (wide nodes x 128 B + leaf points x 16 B + window cells x 16 B + 28 B per query for cloud and winner)."""
    import numpy as np
    crit = api.ICPConvergenceCriteria(0.0, 0.0, args.iters)
    scene = api.Scene_nn().init_Scene_nn_cuda(scene_depth, K)
    for _ in range(2):
        api.refine_batch(model, poses, W, H, proj, K, scene, crit)
    seg = []
    for _ in range(3):                                           # three segments, the median is the figure (see host_solve_extra)
        t0 = time.perf_counter()
        for k in range(steps):                                   # the two slots, like the headline loop: step k is enqueued, then step k-1 collected
            api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
            if k:
                api.refine_wait((k - 1) & 1)
        api.refine_wait((steps - 1) & 1)
        seg.append((time.perf_counter() - t0) / steps)
    dt = sorted(seg)[1]
    # the dominant kernel of this configuration by itself: ONE more batch with events between the four kernels of every pass (profile 3:
    # asynchronous, one pose group, the chip to itself) -> pr_profile_nn
    api.profile_reset()
    api.set_option("profile", 3)
    api.refine_submit(0, model, poses, W, H, proj, K, scene, crit)
    _, sizes_t = api.refine_wait(0)
    api.set_option("profile", 0)
    part_ms, n_pass = api.profile_nn()
    pass_us = api.profile_launches()
    api.set_option("nn_count", 1)
    api.nn_counters(args.iters + 1)
    api.refine_batch(model, poses, W, H, proj, K, scene, crit)
    c = api.nn_counters(args.iters + 1).astype(np.float64)
    api.set_option("nn_count", 0)
    tot = c.sum(0)
    logical = tot[4] * 128 + tot[6] * 16 + tot[7] * 16 + tot[0] * 28          # wide nodes are 128-byte lines, leaf points 16-byte records
    hbm = PMC_TRAFFIC_BYTES_PER_POINT["nn"] * tot[0] if PMC_TRAFFIC_BYTES_PER_POINT["nn"] else None
    roof = None
    if n_pass:
        names = ["nn_search_kernel", "nn_bound_kernel", "nn_tree_wide_kernel<2>", "icp_pass_kernel<SceneNNWinners>"]
        step_ms = float(part_ms.sum())
        k = int(np.argmax(part_ms))
        pts = float(np.sum(sizes_t))                                 # cloud points of the batch = queries of one pass
        walk_s = part_ms[2] * 1e-3 / n_pass
        roof = {"kernel": names[k], "dominant_by": "HIP events between the four kernels of every pass of one timed batch (pr_profile_nn)",
                "avg_launch_us": 1e3 * part_ms[k] / n_pass, "share_of_step": part_ms[k] / step_ms if step_ms > 0 else None,
                "per_kernel_ms_per_step": {n: float(v) for n, v in zip(names, part_ms)}, "passes": int(n_pass), "one_group_step_ms": step_ms,
                "first_passes_us": [float(v) for v in pass_us[:4]],
                "bound": "valu issue + latency (pass 0: 0.47 of the CALIBRATED VALU issue peak -- about 0.6 with its half-rate instructions counted double; rounds 4-5 wrote 0.75 against a peak 1.6x too low -- 539 M wave-instructions for 5.4 M tree searches; a wavefront has a VALU instruction in flight 21 % of its resident cycles, six share a SIMD; HBM ~ 0)",
                "frac": NN_WALK_VALU_ISSUE_FRAC, "frac_of": "VALU issue slots of the chip in pass 0 (the binding resource by the SQ counters; committed pass, see valu_active_frac_source)",
                "valu_issue_frac": NN_WALK_VALU_ISSUE_FRAC,
                "valu_active_frac": NN_WALK_VALU_ACTIVE_FRAC,
                "valu_active_frac_source": "committed: profiles/r06/sq_nn_pass0.txt (nn_tree_wide_kernel, pass 0 of a 256-hypothesis batch: SQ_ACTIVE_INST_VALU 5.39e8, SQ_WAVE_CYCLES 2.6e9, GRBM_GUI_ACTIVE 2.2e7 over 8 XCDs)",
                # HBM side of the task walk alone: committed counter bytes per cloud point x this batch's points over this run's launch time
                "hbm_GBps": (NN_WALK_HBM_BYTES_PER_POINT * pts / walk_s / 1e9) if walk_s > 0 else None,
                "hbm_frac": (NN_WALK_HBM_BYTES_PER_POINT * pts / walk_s / HBM_PEAK) if walk_s > 0 else None,
                "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                "note": "the kd-tree search is cache-resident by design (SURVEY 8d): no kernel of the pass is HBM-bound; hbm_frac is reported because BASELINE's metric asks for it"}
    return {"workload": f"obj_06.ply, {len(poses)}-pose batch, 640x480, kd-tree nearest-neighbour association (Scene_nn: exact search, "
                        "reference tie-breaks; search kernel = keep-the-winner test and pixel-window scan where the bound allows it, bound kernel = "
                        "descent through the representative points + window, task walk over 128-byte wide nodes for the rest, ties repeated by the ordered walk), "
                        f"{args.iters} ICP iterations, two asynchronous slots",
            "value": len(poses) / dt, "unit": "poses/s", "ms_per_step": dt * 1e3, "steps": steps,
            "segments_poses_per_s": [len(poses) / d for d in seg], "value_is": "the median of three consecutive segments of `steps` pipelined steps",
            "roofline": roof,
            "queries_per_step": tot[0], "settled_by_pixel_window_frac": tot[1] / max(tot[0], 1.0), "tree_searches_frac": tot[2] / max(tot[0], 1.0),
            "tree_nodes_per_tree_search": tot[4] / max(tot[2], 1.0), "leaf_points_per_tree_search": tot[6] / max(tot[2], 1.0),
            "logical_bytes_per_step": logical, "logical_GBps_over_step": logical / dt / 1e9,
            "hbm_bytes_per_step_counter": hbm, "hbm_GBps_counter_over_step": (hbm / dt / 1e9) if hbm else None,
            "hbm_frac_of_peak": (hbm / dt / HBM_PEAK) if hbm else None,
            "note": "the kd-tree kernels are cache- and latency-bound by design (SURVEY 8d): their working set (0.85 MB tree + 4.9 MB grid) "
                    "lives in L2, so HBM carries only the clouds and winners; `logical` counts every byte the search asks the caches for"}


def default_criteria_extra(args, api, model, poses, scene_depth, W, H, proj, K, steps=20):
    """"also report default criteria (1e-5, 1e-5, 30)" -- the reference's ICPConvergenceCriteria defaults (icp.h:42-45): a hypothesis
    leaves the loop when fitness and rmse both change by less than 1e-5 (icp.cu:191-194), so hypotheses of a batch drop out at different
    passes (the early-exit path; parity: tests/test_golden_full_gpu.py holds every hypothesis of both scene kinds to the oracle).  Same
    batches, same two-slot loop as the headline, both scene kinds."""
    crit = api.ICPConvergenceCriteria(1e-5, 1e-5, 30)
    out = {"criteria": [1e-5, 1e-5, 30], "note": "reference defaults (icp.h:42-45): per-hypothesis early exit, at most 31 passes; pipelined through the two slots like the headline"}
    for kind in ("proj", "nn"):
        scene = (api.Scene_projective().init_Scene_projective_cuda(scene_depth, K) if kind == "proj" else api.Scene_nn().init_Scene_nn_cuda(scene_depth, K))
        n = steps if kind == "proj" else max(6, steps // 2)
        for k in range(3):
            api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
            if k:
                api.refine_wait((k - 1) & 1)
        api.refine_wait(0)
        t0 = time.perf_counter()
        for k in range(n):
            api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
            if k:
                api.refine_wait((k - 1) & 1)
        api.refine_wait((n - 1) & 1)
        dt = (time.perf_counter() - t0) / n
        out["projective" if kind == "proj" else "kdtree"] = {"value": len(poses) / dt, "unit": "poses/s", "ms_per_step": 1e3 * dt, "steps": n}
    return out


def new_scene_extra(args, api, model, poses, scene_depth, W, H, proj, K, frames=8):
    """SURVEY 8f rank 1 (the reference's README names scene preparation -- normals and the kd-tree build, both on the CPU there -- as what is left
    when the scene changes per frame): a frame = a NEW depth image already in HBM -> scene preparation on the device -> one batch of the headline's
    hypotheses refined against it, synchronously; next to it the same call against an unchanged scene.  Nothing is cached across frames (every frame's
    image differs in a pixel); the scene object keeps its arrays.  tools/scene_frame_time.py splits the figures further."""
    import numpy as np
    crit = api.ICPConvergenceCriteria(0.0, 0.0, args.iters)
    out = {"note": "ms per frame: device scene preparation from a depth image in HBM + one synchronous batch of the headline's hypotheses; `steady_ms`: the same call, scene unchanged",
           "hypotheses": int(len(poses))}
    for kind in ("proj", "nn"):
        scene = api.Scene_projective() if kind == "proj" else api.Scene_nn()
        prep_ms, frame_ms, steady_ms = [], [], []
        for f in range(frames + 2):
            d = np.ascontiguousarray(scene_depth.astype(np.int32))
            d[f % H, f % W] = 0 if d[f % H, f % W] else 905
            dev = api.DeviceVector.from_host(d.reshape(-1))
            api.sync(); t0 = time.perf_counter()
            if kind == "proj": scene.init_Scene_projective_device(dev, K, W, H)
            else: scene.init_Scene_nn_device(dev, K, W, H)
            api.sync(); t1 = time.perf_counter()
            api.refine_batch(model, poses, W, H, proj, K, scene, crit)
            api.sync(); t2 = time.perf_counter()
            api.refine_batch(model, poses, W, H, proj, K, scene, crit)
            api.sync(); t3 = time.perf_counter()
            if f >= 2:
                prep_ms.append(1e3 * (t1 - t0)); frame_ms.append(1e3 * (t2 - t0)); steady_ms.append(1e3 * (t3 - t2))
        out["projective" if kind == "proj" else "kdtree"] = {"frame_ms": float(np.median(frame_ms)), "of_which_preparation_ms": float(np.median(prep_ms)),
                                                             "steady_ms": float(np.median(steady_ms)), "frames": frames,
                                                             "poses_per_s_with_a_new_scene_every_batch": float(len(poses) / (1e-3 * np.median(frame_ms)))}
    return out


def host_solve_extra(args, api, model, poses, W, H, proj, K, scene, steps=30):
    """The same batch with the 6x6 solve ON THE HOST, as `north_star` words it ("SVD solve on host"): per iteration and pose group one launch
    whose last workgroup per hypothesis leaves the 29 sums in pinned host memory, the host solve, and the update read back from pinned
    memory by the next launch (PR_SOLVE_HOST).  The headline keeps the iterations on the device.  Two figures: one host thread issuing
    synchronous calls, and two host threads with private contexts (pr_thread_context) taking the batches in turn -- the reference's own
    suggestion for feeding the GPU ("many host threads, each driving its own pose", README.md:15): one thread's render and host work run
    under the other thread's passes."""
    import threading
    crit = api.ICPConvergenceCriteria(0.0, 0.0, args.iters)
    api.set_option("solve", api.SOLVE_HOST)
    try:
        for _ in range(2):
            api.refine_batch(model, poses, W, H, proj, K, scene, crit)
        t0 = time.perf_counter()
        for _ in range(steps):
            api.refine_batch(model, poses, W, H, proj, K, scene, crit)
        dt_sync = (time.perf_counter() - t0) / steps
        # the same batches pipelined through the two slots from this ONE thread, like the headline loop: with the solve on the host a
        # submitted batch runs on its slot's helper thread (library-owned, private context), so batch k+1's render and host work run under
        # batch k's passes -- the reference's "many host threads" (README.md:15) without the caller having to bring them
        for k in range(4):
            api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
            if k:
                api.refine_wait((k - 1) & 1)
        api.refine_wait(1)
        # three segments of `steps` steps, the MEDIAN segment is the figure (all three are in the line): a 30 ms region catches a one-off stall of
        # 4-6 ms in about one run out of three on this pool's boxes (PR_BENCH_MARKS, round 6: one 6.5 ms step among forty of 1.0 ms, with the solve on
        # either side) -- the median says what the pipeline sustains, the spread what a single short region can read
        seg = []
        for _ in range(3):
            t0 = time.perf_counter()
            for k in range(steps):
                api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
                if k:
                    api.refine_wait((k - 1) & 1)
            api.refine_wait((steps - 1) & 1)
            seg.append((time.perf_counter() - t0) / steps)
        dt = sorted(seg)[1]
        n_threads = 2
        barrier = threading.Barrier(n_threads + 1)
        errors = []

        def work():
            try:
                api.thread_context(True)
                for _ in range(3):
                    api.refine_batch(model, poses, W, H, proj, K, scene, crit)
                barrier.wait()
                for _ in range(steps):
                    api.refine_batch(model, poses, W, H, proj, K, scene, crit)
                barrier.wait()
                api.thread_context(False)
            except Exception as e:                                # noqa: BLE001 -- the figure is an extra: a failure must not cost the line
                errors.append(repr(e))
                barrier.abort()
        ts = [threading.Thread(target=work) for _ in range(n_threads)]
        [t.start() for t in ts]
        try:
            barrier.wait(); t1 = time.perf_counter(); barrier.wait(); dt2 = (time.perf_counter() - t1) / (steps * n_threads)
        except threading.BrokenBarrierError:
            dt2 = None
        [t.join() for t in ts]
    finally:
        api.set_option("solve", api.SOLVE_DEVICE)
    out = {"value": len(poses) / dt, "unit": "poses/s", "ms_per_step": dt * 1e3, "steps": steps, "host_threads": "1 (+2 library: one helper thread per slot)",
           "segments_poses_per_s": [len(poses) / d for d in seg], "value_is": "the median of three consecutive segments of `steps` pipelined steps",
           "group_flags_that_overtook_a_row": int(api.get_option("stat_flag_overtook")),     # (expected 0: the library then waits for the stream instead)
           "note": "PR_SOLVE_HOST, batches pipelined through pr_refine_submit / pr_refine_wait on the two slots from one caller thread; each slot's helper thread runs its batch: 21 launches per pose group (two groups on two streams, software-pipelined: the host solves one group while the other group's pass runs); the workgroup that delivers a hypothesis' last partial sum stores its 29 totals straight into pinned host memory, the one that completes the pose group stores the group's flag behind them; the host polls that flag (round 6: not the stream), solves (pivoted LDLT in double, as Eigen) and the next pass reads the update from the pinned array",
           "one_synchronous_call_per_step": {"value": len(poses) / dt_sync, "unit": "poses/s", "ms_per_step": dt_sync * 1e3, "steps": steps,
                                             "note": "pr_refine_batch in a loop: nothing of batch k+1 can start before batch k has returned"}}
    if dt2:
        out["two_host_threads"] = {"value": len(poses) / dt2, "unit": "poses/s", "ms_per_step": dt2 * 1e3, "steps": steps * n_threads,
                                   "note": "the same synchronous calls from two host threads with private contexts (pr_thread_context), batches taken in turn"}
    elif errors:
        out["two_host_threads"] = {"error": errors[0]}
    return out


def cpu_baseline(args, scene_kind, tris, scene_depth, K, W, H):
    """The CPU oracle (a port of the reference CPU path, oracle/pose_oracle.c at the reference's flags) on a bounded sample of the same
    workload: per-pose render_cpu -> depth2cloud_cpu -> ICP_Point2Plane_cpu with the same fixed 20 iterations, OpenMP across hypotheses
    on the CPUs this process really has (affinity mask capped by the cgroup quota), plus the single-thread rate."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["PR_ORACLE_BUILD"] = "o3"                          # the restatement with the reference's flags (-O3 -fopenmp)
    import oracle_lib as O
    from pose_refine_amd import synth
    usable, facts = effective_cpus()
    threads = int(os.environ.get("PR_BENCH_CPU_THREADS", usable))
    per_pose_s = 0.012 if scene_kind == "proj" else 0.42           # single-thread seconds per hypothesis on the GPU box's host (profiles/r03/cpu_sweep_*.md)
    budget_s = 10.0 if scene_kind == "proj" else 8.0
    n = args.cpu_poses or int(max(2 * threads, min(20000, round(budget_s * threads / per_pose_s))))
    n1 = max(2, int(round((1.5 if scene_kind == "proj" else 1.3) / per_pose_s)))
    oscene = O.ProjScene(scene_depth, K) if scene_kind == "proj" else O.NNScene(scene_depth, K)
    proj = O.compute_proj(K, W, H)
    crit = (0.0, 0.0, args.iters)
    O.set_threads(1)
    t0 = time.perf_counter()
    O.refine_batch(tris, synth.hypotheses(n1), W, H, proj, K, oscene, crit, O.SUM_SEQUENTIAL)
    dt1 = time.perf_counter() - t0
    O.set_threads(threads)
    poses = synth.hypotheses(n)                                     # same seeded stream, longer prefix
    t0 = time.perf_counter()
    _, _, used = O.refine_batch(tris, poses, W, H, proj, K, oscene, crit, O.SUM_SEQUENTIAL)
    dt = time.perf_counter() - t0
    ms_thread, ms_thread1 = 1e3 * dt * used / n, 1e3 * dt1 / n1
    return {"value": n / dt, "unit": "poses/s", "cores": int(used), "kind": "port",
            "sample": f"first {n} hypotheses of the same seeded stream, {dt:.1f} s wall, OpenMP over hypotheses on {used} threads",
            "single_thread": {"value": n1 / dt1, "unit": "poses/s", "sample": f"{n1} hypotheses, {dt1:.1f} s"},
            "ms_per_pose_per_thread": ms_thread, "ms_per_pose_single_thread": ms_thread1, "thread_efficiency": ms_thread1 / ms_thread if ms_thread > 0 else None,
            "host": facts, "threads_rule": "min(affinity mask, cgroup cpu.max quota); PR_BENCH_CPU_THREADS overrides; sweep: profiles/r03/cpu_sweep_*.md",
            "association": "projective" if scene_kind == "proj" else "kd-tree (Scene_nn)",
            "build": "oracle/pose_oracle.c at the reference's flags (-O3 -fopenmp), every thread reusing one depth image and one cloud; per-row check "
                     "against the verbatim reference timings: profiles/r02/cpu_fairness.md"}


if __name__ == "__main__":
    sys.exit(main())
