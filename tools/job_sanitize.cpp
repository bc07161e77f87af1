// build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Wno-unused-result -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Ipose_refine_amd/csrc tools/job_sanitize.cpp -o job_sanitize;  ./job_sanitize
// Sanitizer harness for the host-only helpers of the fused batch path and the scoring path (pr_runtime.h): make_job, score_request_ok, render_args_ok and vsd_args_ok with null and
// out-of-range arguments, the layouts of a slot's pinned blocks (SlotIn, SlotOut) and of the kd-tree workspace (nn_layout, nn_carve), the pose-group split; the packed layouts (box_area, box_slot, cloud_slot), the plan of an asynchronous batch (plan_async), the overlap rule (release_pass_for) the byte rule of a timed pass (icp_span_bytes), the mixed-batch layer (plan_meshes on a worked example and on every table it refuses; Batch: gather, scatter, the pyramid's rows, the P x P matrix, the inverse, the one-mesh identity; camera_centers bit for bit against the expression it replaced), pose observability's argument checks and covariance (info_scene_ok, info_center_radius_ok, info_covariance), and the scene caches (the control words NNInfo and the fingerprint words FpWords / ProjTail at their documented positions, packed_layout, the source lists scene_sources / check_sources, pick_nn_set rule by rule, nn_route at every clamp), and the frame stages' shared rules and layouts (frame_stage.h: depth_frame_ok, gate_ok, window_ok, with_depth, Block, ScanRows and the blocks of the planes, segments and PPF votes at their smallest and largest parameters).  None of them calls HIP, so nothing of the runtime is linked.
#include <cstdio>
#include "pr_runtime.h"
#include "frame_stage.h"
namespace prh { void set_error(const char *, ...) {} }
using namespace prr;
static long fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)
int main()
{
    const pr_triangle *tris = reinterpret_cast<const pr_triangle *>(uintptr_t(0x1000));     // never dereferenced: the job keeps addresses of device memory
    pr_vec3 *dev = reinterpret_cast<pr_vec3 *>(uintptr_t(0x2000));
    const float K[9] = { 500, 0, 320, 0, 500, 240, 0, 0, 1 };
    pr_mat4 proj{};
    pr_scene_proj sp{}; sp.pcd = dev; sp.normal = dev; sp.width = 640; sp.height = 480; sp.max_dist_diff = 10.0f;
    pr_scene_proj_crop sc{}; sc.view = sp; sc.tl_x = 7; sc.tl_y = 9;
    pr_scene_nn sn{}; sn.pcd = dev; sn.normal = dev; sn.n_points = 11;
    const pr_criteria crit{ 0.0f, 0.0f, 2 };
    const pr_roi none{ 0, 0, 0, 0 };
    pr_result *rdev = reinterpret_cast<pr_result *>(uintptr_t(0x3000));
    RefineJob job;
    // what must be refused, one mistake at a time; `job` stays as it was
    job.W = 77;
    auto refused = [&](const pr_triangle *t, size_t nt, uint32_t W, uint32_t H, const pr_mat4 *p, const float *k, int kind, const void *s, pr_criteria c, pr_roi r) {
        CHECK(make_job("job_sanitize", t, nt, W, H, p, k, kind, s, c, r, nullptr, job) == PR_ERR_INVALID);
        CHECK(job.W == 77);
    };
    refused(nullptr, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none);
    refused(tris, 5, 640, 480, nullptr, K, PR_SCENE_PROJ, &sp, crit, none);
    refused(tris, 5, 640, 480, &proj, nullptr, PR_SCENE_PROJ, &sp, crit, none);
    for (int kind : { PR_SCENE_PROJ, PR_SCENE_NN, PR_SCENE_PROJ_CROP }) refused(tris, 5, 640, 480, &proj, K, kind, nullptr, crit, none);
    for (int kind : { -1, 4, 1 << 30, -2147483647 - 1 }) refused(tris, 5, 640, 480, &proj, K, kind, &sp, crit, none);
    // a closest-point grid: one mistake at a time in an otherwise good description
    pr_scene_grid sg{};
    sg.cell = 0.25f; sg.inv_cell = 4.0f; sg.dim[0] = 4; sg.dim[1] = 5; sg.dim[2] = 6; sg.max_dist_diff = 0.1f; sg.reach = 0.3f; sg.n_points = 11;
    sg.cell_point = reinterpret_cast<const uint32_t *>(uintptr_t(0xd000)); sg.rec = reinterpret_cast<const float *>(uintptr_t(0xf000));
    refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, nullptr, crit, none);
    { pr_scene_grid b = sg; b.cell_point = nullptr; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.rec = nullptr; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.inv_cell = 3.9999998f; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.cell = 0.0f; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.cell = -0.25f; b.inv_cell = -4.0f; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.cell = NAN; b.inv_cell = NAN; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.origin[1] = INFINITY; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.dim[2] = 0; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.dim[0] = 1u << 13; b.dim[1] = 1u << 13; b.dim[2] = 2; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }      // 2^27 cells
    { pr_scene_grid b = sg; b.dim[0] = 0xffffffffu; b.dim[1] = 0xffffffffu; b.dim[2] = 0xffffffffu; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.max_dist_diff = 0.0f; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.reach = NAN; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.n_points = 0; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    { pr_scene_grid b = sg; b.n_points = 1u << 27; refused(tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none); }
    refused(tris, 5, 0, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none);
    refused(tris, 5, 640, 0, &proj, K, PR_SCENE_PROJ, &sp, crit, none);
    refused(tris, 5, 8193, 1, &proj, K, PR_SCENE_PROJ, &sp, crit, none);
    refused(tris, 5, 8192, 4096, &proj, K, PR_SCENE_PROJ, &sp, crit, none);              // 2^25 pixels
    refused(tris, 5, 0xffffffffu, 0xffffffffu, &proj, K, PR_SCENE_PROJ, &sp, crit, none);
    refused(tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, pr_criteria{ 0.0f, 0.0f, -1 }, none);
    for (pr_roi r : { pr_roi{ -1, 0, 10, 10 }, pr_roi{ 0, -1, 10, 10 }, pr_roi{ 631, 0, 10, 10 }, pr_roi{ 0, 471, 10, 10 }, pr_roi{ 2147483647, 0, 2147483647, 1 },
                      pr_roi{ 0, 2147483647, 1, 2147483647 } })
        refused(tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, r);
    // what must pass, and what the job then holds
    CHECK(make_job("job_sanitize", nullptr, 0, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, rdev, job) == PR_OK);      // an empty model has no array
    CHECK(job.mesh.tris == nullptr && job.mesh.n_tris == 0 && job.mesh.plan == nullptr && job.W == 640 && job.H == 480 && job.results_dev == rdev && job.K[4] == 500.0f);
    CHECK(job.scene() == &job.sp && job.sp.view.width == 640 && job.sp.tl_x == 0 && job.sp.tl_y == 0);
    CHECK(make_job("job_sanitize", tris, 5, 8192, 2048, &proj, K, PR_SCENE_PROJ_CROP, &sc, pr_criteria{ 1e-5f, 1e-5f, 0 }, pr_roi{ 630, 470, 10, 10 }, nullptr, job) == PR_OK);
    CHECK(job.scene() == &job.sp && job.sp.tl_x == 7 && job.sp.tl_y == 9 && job.roi.x == 630 && job.crit.max_iteration == 0 && job.results_dev == nullptr);
    CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_NN, &sn, crit, pr_roi{ 5, 5, -3, 0 }, nullptr, job) == PR_OK);       // (no ROI)
    CHECK(job.scene() == &job.sn && job.sn.n_points == 11);
    { pr_scene_grid b = sg; b.dim[0] = 1u << 13; b.dim[1] = 1u << 13; b.dim[2] = 1;                                    // exactly PR_GRID_MAX_CELLS
      CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_GRID, &b, crit, none, nullptr, job) == PR_OK); }
    CHECK(job.scene() == &job.sg && job.sg.dim[0] == (1u << 13) && job.sg.cell_point == sg.cell_point && job.sg.n_points == 11);
    CHECK(grid_desc_ok("job_sanitize", &sg, false) == PR_OK && grid_desc_ok("job_sanitize", nullptr, false) == PR_ERR_INVALID);
    { pr_scene_grid b = sg; b.cell_point = nullptr; b.rec = nullptr; b.n_points = 0; CHECK(grid_desc_ok("job_sanitize", &b, false) == PR_OK); }      // (as pr_scene_grid_describe leaves it: good for the build)
    // robust tables (pr_robust): one descriptor for every level or one per level, each as pr_robust_describe would have made it
    {
        const pr_robust huber{ PR_ROBUST_HUBER, 0.02f, 1.0f / 0.02f, 0 }, tukey{ PR_ROBUST_TUKEY, 0.005f, 1.0f / 0.005f, 0 }, plain{ PR_ROBUST_NONE, 0.0f, 0.0f, 0 };
        const pr_robust two[2] = { huber, tukey };
        CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, two, 2, 2) == PR_OK);
        CHECK(job.robust[0].kind == PR_ROBUST_HUBER && job.robust[1].kind == PR_ROBUST_TUKEY && job.robust[1].inv_c == two[1].inv_c && job.robust[2].kind == PR_ROBUST_NONE);
        CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, &tukey, 1, 3) == PR_OK);
        CHECK(job.robust[0].kind == PR_ROBUST_TUKEY && job.robust[2].kind == PR_ROBUST_TUKEY && job.robust[3].kind == PR_ROBUST_NONE);
        CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, &plain, 1, 1) == PR_OK && job.robust[0].kind == PR_ROBUST_NONE);
        CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job) == PR_OK && job.robust[0].kind == PR_ROBUST_NONE);
        for (uint32_t n_robust : { 0u, 2u, 4u, 5u })              // neither 1 nor the 3 levels
            CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, two, n_robust, 3) == PR_ERR_INVALID);
        CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, nullptr, 1, 1) == PR_ERR_INVALID);
        CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, two, 2, 5) == PR_ERR_INVALID);      // more levels than a pyramid has
        for (pr_robust bad : { pr_robust{ 4, 0.02f, 50.0f, 0 }, pr_robust{ PR_ROBUST_HUBER, 0.02f, 1.0f / 0.02f, 1 }, pr_robust{ PR_ROBUST_HUBER, 0.0f, 0.0f, 0 },
                               pr_robust{ PR_ROBUST_TUKEY, -0.02f, -50.0f, 0 }, pr_robust{ PR_ROBUST_CAUCHY, NAN, 50.0f, 0 }, pr_robust{ PR_ROBUST_CAUCHY, INFINITY, 0.0f, 0 },
                               pr_robust{ PR_ROBUST_HUBER, 0.02f, std::nextafter(1.0f / 0.02f, 0.0f), 0 } }) {     // (the last: an inv_c one ulp off 1.0f / c)
            const pr_robust with_bad[2] = { huber, bad };
            CHECK(robust_desc_ok("job_sanitize", &bad) == PR_ERR_INVALID);
            CHECK(make_job("job_sanitize", tris, 5, 640, 480, &proj, K, PR_SCENE_PROJ, &sp, crit, none, nullptr, job, with_bad, 2, 2) == PR_ERR_INVALID);
        }
        CHECK(robust_desc_ok("job_sanitize", nullptr) == PR_ERR_INVALID && robust_desc_ok("job_sanitize", &huber) == PR_OK);
    }
    // scoring requests: one good one per kind, single mesh and mesh table; then one mistake at a time -- a null array, too many hypotheses, a ROI off the frame
    const pr_mat4 *poses = reinterpret_cast<const pr_mat4 *>(uintptr_t(0x4000));
    const pr_mesh_ref *table = reinterpret_cast<const pr_mesh_ref *>(uintptr_t(0x5000));
    const uint32_t *index = reinterpret_cast<const uint32_t *>(uintptr_t(0x6000));
    pr_pose_score *scores = reinterpret_cast<pr_pose_score *>(uintptr_t(0x7000));
    uint32_t *matrix = reinterpret_cast<uint32_t *>(uintptr_t(0x8000));
    const uint8_t *edges = reinterpret_cast<const uint8_t *>(uintptr_t(0x9000));
    pr_pose_contour *contours = reinterpret_cast<pr_pose_contour *>(uintptr_t(0xa000));
    pr_pose_visible *visible = reinterpret_cast<pr_pose_visible *>(uintptr_t(0xb000));
    pr_frame_explained *frame = reinterpret_cast<pr_frame_explained *>(uintptr_t(0xc000));
    const pr_roi off_frame{ 631, 0, 10, 10 };
    pr_pose_normal *normals = reinterpret_cast<pr_pose_normal *>(uintptr_t(0xe000));
    for (ScoreKind kind : { kScorePoses, kScoreOverlap, kScoreContours, kScoreNormals, kScoreCompose })
        for (bool multi : { false, true }) {
            ScoreRequest ok{};
            ok.fn = "job_sanitize"; ok.kind = kind; ok.mesh = multi ? MeshArg::table(table, 2, index) : MeshArg::one(tris, 5); ok.poses = poses; ok.P = 70; ok.W = 640; ok.H = 480; ok.proj = &proj; ok.roi = pr_roi{ 630, 470, 10, 10 };
            ok.scene = dev; ok.scene_i32 = true; ok.tau = 0; ok.scores = scores;
            if (kind == kScoreOverlap) ok.overlap = matrix;
            if (kind == kScoreContours) { ok.jump = 0; ok.edge_dist = edges; ok.contours = contours; }       // (no matrix: it is optional here)
            if (kind == kScoreNormals) { ok.K = K; ok.step = PR_NORMAL_MAX_STEP; ok.jump = 0; ok.cos_min = 1.0f; ok.normals = normals; }       // (no matrix: it is optional here)
            if (kind == kScoreCompose) { ok.visible = visible; ok.frame = frame; }                          // (neither image: both are optional)
            CHECK(score_request_ok(ok) == PR_OK);
            ScoreRequest none_to_score = ok; none_to_score.P = 0; none_to_score.poses = nullptr; none_to_score.scene = nullptr; none_to_score.scores = nullptr;
            none_to_score.overlap = nullptr; none_to_score.edge_dist = nullptr; none_to_score.contours = nullptr; none_to_score.K = nullptr; none_to_score.normals = nullptr; none_to_score.visible = nullptr; none_to_score.frame = nullptr;
            CHECK(score_request_ok(none_to_score) == PR_OK);                                               // no hypotheses need no arrays
            auto refused_with = [&](auto &&mistake) { ScoreRequest r = ok; mistake(r); CHECK(score_request_ok(r) == PR_ERR_INVALID); };
            refused_with([](ScoreRequest &r) { r.poses = nullptr; });
            refused_with([](ScoreRequest &r) { r.scene = nullptr; });
            refused_with([](ScoreRequest &r) { r.scores = nullptr; });
            refused_with([](ScoreRequest &r) { r.proj = nullptr; });
            refused_with([](ScoreRequest &r) { r.tau = -1; });
            refused_with([&](ScoreRequest &r) { r.roi = off_frame; });
            refused_with([](ScoreRequest &r) { r.roi = pr_roi{ 2147483647, 0, 2147483647, 1 }; });
            refused_with([](ScoreRequest &r) { r.W = 8193; r.H = 1; });
            refused_with([](ScoreRequest &r) { r.W = 0xffffffffu; r.H = 0xffffffffu; });
            refused_with([](ScoreRequest &r) { r.W = 0; });
            if (!multi) refused_with([](ScoreRequest &r) { r.mesh.tris = nullptr; });
            if (kind == kScoreOverlap) refused_with([](ScoreRequest &r) { r.overlap = nullptr; });
            if (kind == kScoreOverlap) refused_with([](ScoreRequest &r) { r.P = PR_OVERLAP_MAX_POSES + 1; });
            if (kind == kScoreContours) {
                refused_with([](ScoreRequest &r) { r.edge_dist = nullptr; });
                refused_with([](ScoreRequest &r) { r.contours = nullptr; });
                refused_with([](ScoreRequest &r) { r.jump = -2147483647 - 1; });
                refused_with([&](ScoreRequest &r) { r.overlap = matrix; r.P = PR_OVERLAP_MAX_POSES + 1; });
                ScoreRequest many = ok; many.P = PR_OVERLAP_MAX_POSES + 1;                                    // without a matrix there is no such limit
                CHECK(score_request_ok(many) == PR_OK);
            }
            if (kind == kScoreNormals) {
                refused_with([](ScoreRequest &r) { r.K = nullptr; });
                refused_with([](ScoreRequest &r) { r.normals = nullptr; });
                refused_with([](ScoreRequest &r) { r.step = 0; });
                refused_with([](ScoreRequest &r) { r.step = PR_NORMAL_MAX_STEP + 1; });
                refused_with([](ScoreRequest &r) { r.step = 0xffffffffu; });
                refused_with([](ScoreRequest &r) { r.jump = -1; });
                refused_with([](ScoreRequest &r) { r.jump = -2147483647 - 1; });
                for (float c : { -1e-6f, 1.0001f, NAN, INFINITY, -INFINITY }) refused_with([c](ScoreRequest &r) { r.cos_min = c; });
                refused_with([&](ScoreRequest &r) { r.overlap = matrix; r.P = PR_OVERLAP_MAX_POSES + 1; });
                ScoreRequest many = ok; many.P = PR_OVERLAP_MAX_POSES + 1; many.cos_min = 0.0f; many.step = 1; many.jump = 2147483647;      // without a matrix there is no such limit
                CHECK(score_request_ok(many) == PR_OK);
                ScoreRequest none_bad = none_to_score; none_bad.step = 0;                                       // the estimator's parameters are checked whatever P is
                CHECK(score_request_ok(none_bad) == PR_ERR_INVALID);
            }
            if (kind == kScoreCompose) {
                refused_with([](ScoreRequest &r) { r.visible = nullptr; });
                refused_with([](ScoreRequest &r) { r.frame = nullptr; });
                refused_with([](ScoreRequest &r) { r.P = PR_COMPOSE_MAX_POSES + 1; });
                CHECK(compose_args_ok("job_sanitize", PR_COMPOSE_MAX_POSES) == PR_OK && compose_args_ok("job_sanitize", 0xffffffffu) == PR_ERR_INVALID);
            }
        }
    // pr_pose_vsd's arguments: a good call of each form, nothing to compute, then one mistake at a time (the poses are read: real arrays)
    {
        std::vector<pr_mat4> est(5), gt(5);
        for (auto *v : { &est, &gt }) for (pr_mat4 &m : *v) identity16(m.m);
        const float taus[PR_VSD_MAX_TAUS + 1] = { 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
        pr_vsd_counts *out = reinterpret_cast<pr_vsd_counts *>(uintptr_t(0xd000));
        auto vsd = [&](bool multi, const pr_triangle *t, const pr_mat4 *e, uint32_t ne, const pr_mat4 *gp, uint32_t ng, uint32_t W, uint32_t H, const pr_mat4 *p, const void *s,
                       const float *k, float delta, const float *ts, uint32_t nt, const pr_vsd_counts *o) {
            return vsd_args_ok("job_sanitize", multi, t, 5, e, ne, gp, ng, W, H, p, s, k, delta, ts, nt, o);
        };
        for (bool multi : { false, true }) {
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, PR_VSD_MAX_TAUS, out) == PR_OK);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, nullptr, 0.0f, nullptr, 0, out) == PR_OK);
            CHECK(vsd(multi, nullptr, nullptr, 0, nullptr, 0, 640, 480, nullptr, nullptr, nullptr, 15.0f, nullptr, 3, nullptr) == PR_OK);       // no pairs need no arrays
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 1, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == (multi ? PR_ERR_INVALID : PR_OK));
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 4, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 0, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 0x80000000u, gt.data(), 0x80000000u, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, PR_VSD_MAX_TAUS + 1, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, 0xffffffffu, out) == PR_ERR_INVALID);
            for (float bad : { -1.0f, -0.0f - 1e-30f, INFINITY, -INFINITY, NAN }) {
                CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, bad, taus, 3, out) == PR_ERR_INVALID);
                float t3[3] = { 1.0f, bad, 3.0f };
                CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, t3, 3, out) == PR_ERR_INVALID);
                float k9[9]; std::memcpy(k9, K, sizeof k9); k9[7] = bad;
                if (!std::isfinite(bad)) CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, k9, 15.0f, taus, 3, out) == PR_ERR_INVALID);
                std::vector<pr_mat4> e2 = est; e2[4].m[15] = bad;
                if (!std::isfinite(bad)) CHECK(vsd(multi, tris, e2.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
                if (!std::isfinite(bad)) CHECK(vsd(multi, tris, est.data(), 5, e2.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            }
            const float down[3] = { 1.0f, 3.0f, 2.0f };
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, down, 3, out) == PR_ERR_INVALID);
            for (int i : { 0, 4 }) {
                float k9[9]; std::memcpy(k9, K, sizeof k9); k9[i] = 0.0f;
                CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, k9, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            }
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, nullptr, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, nullptr, 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, nullptr, 5, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, nullptr, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, nullptr, 3, out) == PR_ERR_INVALID);
            CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, 3, nullptr) == PR_ERR_INVALID);
            CHECK(vsd(multi, nullptr, est.data(), 5, gt.data(), 5, 640, 480, &proj, dev, K, 15.0f, taus, 3, out) == (multi ? PR_OK : PR_ERR_INVALID));
            for (auto [W, H] : { std::pair<uint32_t, uint32_t>{ 0, 480 }, { 640, 0 }, { 8193, 1 }, { 8192, 4096 }, { 0xffffffffu, 0xffffffffu } })
                CHECK(vsd(multi, tris, est.data(), 5, gt.data(), 5, W, H, &proj, dev, K, 15.0f, taus, 3, out) == PR_ERR_INVALID);
        }
    }
    // the full-frame renders' arguments (render_args_ok): plain, span and mixed; nothing to render needs no arrays; a far plane only where one is written
    {
        const int32_t *plane = reinterpret_cast<const int32_t *>(uintptr_t(0xd000));
        for (bool multi : { false, true })
            for (bool span : { false, true }) {
                auto render = [&](const pr_triangle *t, const pr_mat4 *p, size_t P, size_t W, size_t H, const pr_mat4 *pj, pr_roi r, const int32_t *n, const int32_t *f) {
                    return render_args_ok("job_sanitize", multi, span, t, 5, p, P, W, H, pj, r, n, f);
                };
                CHECK(render(tris, poses, 70, 640, 480, &proj, pr_roi{ 630, 470, 10, 10 }, plane, plane) == PR_OK);
                CHECK(render(tris, nullptr, 0, 640, 480, &proj, none, nullptr, nullptr) == PR_OK);
                CHECK(render(tris, poses, 70, 640, 480, &proj, none, plane, nullptr) == (span ? PR_ERR_INVALID : PR_OK));
                CHECK(render(nullptr, poses, 70, 640, 480, &proj, none, plane, plane) == (multi ? PR_OK : PR_ERR_INVALID));
                CHECK(render(tris, nullptr, 70, 640, 480, &proj, none, plane, plane) == PR_ERR_INVALID && render(tris, poses, 70, 640, 480, &proj, none, nullptr, plane) == PR_ERR_INVALID);
                CHECK(render(tris, poses, 70, 640, 480, nullptr, none, plane, plane) == PR_ERR_INVALID && render(tris, poses, 70, 640, 480, &proj, off_frame, plane, plane) == PR_ERR_INVALID);
                for (auto [W, H] : { std::pair<size_t, size_t>{ 0, 480 }, { 640, 0 }, { 8193, 1 }, { 8192, 4096 }, { size_t(1) << 40, size_t(1) << 40 } })
                    CHECK(render(tris, poses, 70, W, H, &proj, none, plane, plane) == PR_ERR_INVALID);
                CHECK(render(tris, poses, size_t(1) << 32, 640, 480, &proj, none, plane, plane) == (multi ? PR_ERR_INVALID : PR_OK));
            }
    }
    // the pinned blocks of a slot: the parts in order, none overlapping, written and read back over their whole length
    for (size_t P : { size_t(0), size_t(1), size_t(3), size_t(65) }) {
        const SlotIn in(P);
        CHECK(in.box == sizeof(pr_mat4) * P && in.off == in.box + sizeof(int4) * P && in.bytes == in.off + sizeof(uint32_t) * P);
        CHECK(in.box % alignof(int4) == 0 && in.off % alignof(uint32_t) == 0);
        const SlotOut out(P);
        CHECK(out.res >= sizeof(uint32_t) * P && out.res % 64 == 0 && out.flag >= out.res + sizeof(pr_result) * P && out.flag % 64 == 0 && out.bytes == out.flag + 64);
        CHECK(out.res < sizeof(uint32_t) * P + 64 && out.flag < out.res + sizeof(pr_result) * P + 64);
        std::vector<unsigned char> hin(in.bytes + 16), hout(out.bytes);
        for (size_t i = 0; i < P; ++i) {
            reinterpret_cast<pr_mat4 *>(hin.data())[i] = proj;
            reinterpret_cast<int4 *>(hin.data() + in.box)[i] = int4{ 1, 2, 3, 4 };
            reinterpret_cast<uint32_t *>(hin.data() + in.off)[i] = (uint32_t)i;
            reinterpret_cast<uint32_t *>(hout.data())[i] = (uint32_t)i;
            reinterpret_cast<pr_result *>(hout.data() + out.res)[i] = pr_result{};
        }
        *reinterpret_cast<uint32_t *>(hout.data() + out.flag) = 1u;
        for (size_t i = 0; i < P; ++i) CHECK(reinterpret_cast<uint32_t *>(hin.data() + in.off)[i] == i && reinterpret_cast<uint32_t *>(hout.data())[i] == i);
        // ... and the pose groups of that many hypotheses: consecutive, complete, at most four
        for (uint32_t n_groups = 1; n_groups <= 4; ++n_groups) {
            CHECK(group_begin((uint32_t)P, n_groups, 0) == 0 && group_begin((uint32_t)P, n_groups, n_groups) == P);
            for (uint32_t k = 0; k < n_groups; ++k) CHECK(group_begin((uint32_t)P, n_groups, k) <= group_begin((uint32_t)P, n_groups, k + 1));
        }
    }
    // the kd-tree workspace: the five regions in order and disjoint, both queues on 8 bytes, the counters at word 6 x span, the size the drivers
    // always asked for; carved from a block of that size, the last word of every region is inside it
    for (size_t span : { size_t(1), size_t(31), size_t(32), size_t(1) << 20, (size_t(1) << 30) - 1 })
        for (size_t P : { size_t(1), size_t(32768) }) {
            const NNLayout l = nn_layout(span, P);
            CHECK(l.winners == 0 && l.winners + span <= l.slack && l.slack + span <= l.queue && l.queue + 2 * span <= l.queue2 && l.queue2 + 2 * span <= l.qcount);
            CHECK(l.qcount == 6 * span && sizeof(uint32_t) * (l.qcount + prk::kQCountStride * P) <= l.bytes);
            CHECK(l.bytes == 4 * (6 * span + 4 * P) + 64);
            uint32_t *base = static_cast<uint32_t *>(std::malloc(l.bytes));
            CHECK(base != nullptr);
            if (!base) continue;
            prk::IcpBatch b{};
            nn_carve(b, base, l);
            CHECK(b.nn_prev == base && reinterpret_cast<uint32_t *>(b.nn_slack) == base + l.slack && b.nn_qcount == base + l.qcount);
            CHECK(reinterpret_cast<uintptr_t>(b.nn_queue) % alignof(uint2) == 0 && reinterpret_cast<uintptr_t>(b.nn_queue2) % alignof(uint2) == 0);
            CHECK(reinterpret_cast<uintptr_t>(b.nn_queue) % 8 == 0 && reinterpret_cast<uintptr_t>(b.nn_queue2) % 8 == 0);
            b.nn_prev[span - 1] = 1u; b.nn_slack[span - 1] = 2.0f; b.nn_queue[span - 1] = uint2{ 3u, 4u }; b.nn_queue2[span - 1] = uint2{ 5u, 6u };
            b.nn_qcount[prk::kQCountStride * P - 1] = 7u;
            CHECK(b.nn_prev[span - 1] == 1u && b.nn_slack[span - 1] == 2.0f && b.nn_queue[span - 1].y == 4u && b.nn_queue2[span - 1].x == 5u && b.nn_qcount[prk::kQCountStride * P - 1] == 7u);
            std::free(base);
        }
    CHECK(group_begin(0xffffffffu, 4, 4) == 0xffffffffu && group_begin(0xffffffffu, 4, 3) == 0xbfffffffu);
    // the packed layouts: an empty or inverted box has no pixels; a slot is a multiple of 32, never smaller than what it holds and less than 32 larger
    static_assert(prk::kBoxPack == 32 && prk::kCloudAlign == 32, "the values below are written for slots of 32");
    CHECK(prk::box_area(int4{ 0, 0, 0, 0 }) == 1 && prk::box_area(int4{ 3, 5, 12, 5 }) == 10 && prk::box_area(int4{ 0, 0, 4095, 4095 }) == (1u << 24));
    for (int4 b : { int4{ 5, 0, 4, 9 }, int4{ 0, 5, 9, 4 }, int4{ 9, 9, 0, 0 }, int4{ 0, 0, -1, -1 }, int4{ 8191, 0, -8191, 0 }, int4{ 100, 100, 3, 200 } }) CHECK(prk::box_area(b) == 0);
    {
        const uint32_t in[6] = { 0u, 1u, 31u, 32u, 33u, 0xffffffdfu }, want[6] = { 0u, 32u, 32u, 32u, 64u, 0xffffffe0u };      // (the last: 2^32 - 33)
        for (int k = 0; k < 6; ++k)
            for (uint32_t got : { prk::box_slot(in[k]), prk::cloud_slot(in[k]) }) CHECK(got == want[k] && got % 32 == 0 && got >= in[k] && got - in[k] < 32);
    }
    // plan_async: the sub-batch split ...
    {
        auto plan_of = [](uint32_t P, uint32_t W, uint32_t H, int4 box, int sub_batch, uint32_t hint = 0, int steps = 3) {
            std::vector<int4> boxes(P, box); std::vector<uint32_t> off(P, 0xdeadbeefu);
            return plan_async(P, W, H, boxes.data(), steps, sub_batch, hint, off.data());
        };
        const int4 small{ 10, 10, 73, 41 };                                                              // 64 x 32 pixels
        { const AsyncPlan pl = plan_of(96, 640, 480, small, 40); CHECK(pl.n_sub == 3 && pl.sub == 32); }
        { const AsyncPlan pl = plan_of(96, 640, 480, small, 64); CHECK(pl.n_sub == 2 && pl.sub == 48); }
        { const AsyncPlan pl = plan_of(512, 4096, 4096, small, 512); CHECK(pl.sub == 64 && pl.n_sub == 8); }                  // 4 GiB / 64 MiB
        { const AsyncPlan pl = plan_of(512, 2048, 1024, small, 512); CHECK(pl.sub == 512 && pl.n_sub == 1); }                 // 2 M pixels
        { const AsyncPlan pl = plan_of(1024, 640, 480, int4{ 0, 0, 639, 479 }, 512); CHECK(pl.sub == 512 && pl.n_sub == 2); }
        { const AsyncPlan pl = plan_of(7, 640, 480, int4{ 9, 9, 0, 0 }, 512); CHECK(pl.max_area == 1 && pl.cstride == 32 && pl.nblk == 1 && pl.grid_x == 1); }      // all boxes empty
    }
    // ... and the layout: boxes of many sizes, empty ones among them, over several frames, sub-batch sizes, step counts and cloud hints
    for (auto [W, H] : { std::pair<uint32_t, uint32_t>{ 96, 260 }, { 640, 480 }, { 1, 1 }, { 4096, 4096 } })
        for (uint32_t P : { 1u, 31u, 96u, 257u, 513u })
            for (int sub_batch : { 1, 40, 512 })
                for (uint32_t hint : { 0u, 1u, 5000u, 1u << 24 })                                   // (a cloud has at most 2^24 points: frame_size_ok)
                    for (int steps : { 0, 1, 3 }) {
                        std::vector<int4> boxes(P); std::vector<uint32_t> off(P, 0xdeadbeefu);
                        uint32_t x = 12345u * W + P;
                        auto next = [&](uint32_t m) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % m); };
                        for (int4 &b : boxes) { b = int4{ next(W), next(H), next(W), next(H) }; if (next(5) == 0) b = int4{ 0, 0, (int)W - 1, (int)H - 1 }; }   // (inverted about half of the time; the whole frame now and then)
                        const AsyncPlan pl = plan_async(P, W, H, boxes.data(), steps, sub_batch, hint, off.data());
                        size_t largest = 1;
                        for (const int4 &b : boxes) largest = std::max<size_t>(largest, prk::box_area(b));
                        CHECK(pl.max_area == largest && pl.cstride >= pl.max_area && pl.cstride % prk::kCloudAlign == 0);
                        CHECK(pl.steps == (uint32_t)std::max(1, steps) && (size_t)pl.nblk * pl.steps * prk::kPointsPerStep >= pl.max_area);
                        CHECK(pl.grid_x >= 1 && pl.grid_x <= pl.nblk && (hint != 0 || pl.grid_x == pl.nblk));
                        CHECK(pl.sub >= 1 && pl.n_sub >= 1 && (size_t)pl.sub * pl.n_sub >= P && (size_t)pl.sub * (pl.n_sub - 1) < P && pl.sub <= (uint32_t)std::max(32, sub_batch));
                        CHECK((size_t)pl.sub * W * H * sizeof(int32_t) <= ((size_t)4 << 30) && (size_t)pl.sub * pl.cstride <= ((size_t)1 << 30));
                        for (uint32_t i = 0; i < P; ++i) {
                            CHECK(off[i] % prk::kBoxPack == 0);
                            if (i % pl.sub == 0) CHECK(off[i] == 0);
                            else CHECK(off[i] >= off[i - 1] && off[i] == off[i - 1] + prk::box_slot(prk::box_area(boxes[i - 1])));
                            if ((i + 1) % pl.sub == 0 || i + 1 == P) CHECK((size_t)off[i] + prk::box_area(boxes[i]) <= ((size_t)W * H + prk::kBoxPack) * pl.sub);
                        }
                        // the same boxes in the banded layout (option box_bands): slots from box_slot_of, the workspace bound with the height rounded up to 4
                        const AsyncPlan pb = plan_async(P, W, H, boxes.data(), steps, sub_batch, hint, off.data(), /*bands=*/true);
                        CHECK(pb.max_area == pl.max_area && pb.cstride == pl.cstride && pb.nblk == pl.nblk && pb.grid_x == pl.grid_x && pb.sub >= 1 && pb.sub <= pl.sub);
                        CHECK((size_t)pb.sub * W * ((H + 3) & ~3u) * sizeof(int32_t) <= ((size_t)4 << 30));
                        for (uint32_t i = 0; i < P; ++i) {
                            const uint32_t ints = prk::box_ints(boxes[i], H, true);
                            CHECK(off[i] % prk::kBoxPack == 0 && ints % 4 == 0 && ints >= prk::box_area(boxes[i]) && (prk::box_area(boxes[i]) > 0 || ints == 0));
                            if (i % pb.sub == 0) CHECK(off[i] == 0);
                            else CHECK(off[i] == off[i - 1] + prk::box_slot_of(boxes[i - 1], H, true));
                            if ((i + 1) % pb.sub == 0 || i + 1 == P) CHECK((size_t)off[i] + ints <= depth_ints_per_pose(W, H, true) * pb.sub);
                        }
                    }
    // release_pass_for: the measured rule at the benchmark's figures, the scene kinds, a timed batch, the two options
    {
        const pr_criteria c20{ 0.0f, 0.0f, 20 };
        auto rule = [&](uint32_t nq, int kind = PR_SCENE_PROJ, bool timed = false, bool start = false, int start_overlap = -1, int overlap_pass = -1) {
            return release_pass_for(31468, nq, 27400, c20, kind, timed, start, start_overlap, overlap_pass);
        };
        CHECK(rule(128) == 0 && rule(256) == 8 && rule(384) == 14 && rule(512) == 16);
        CHECK(rule(128, PR_SCENE_PROJ_CROP) == 0 && rule(512, PR_SCENE_PROJ_CROP) == 16);
        for (uint32_t nq : { 128u, 256u, 384u, 512u }) CHECK(rule(nq, PR_SCENE_NN) == 0 && rule(nq, PR_SCENE_PROJ, /*timed=*/true) == 20 && rule(nq, PR_SCENE_NN, true, true, 2, 3) == 20);
        CHECK(rule(512, PR_SCENE_PROJ, false, false, -1, 3) == 3 && rule(512, PR_SCENE_PROJ, false, true, -1, 3) == 3 && rule(512, PR_SCENE_NN, false, false, -1, 3) == 3);
        CHECK(rule(512, PR_SCENE_PROJ, false, true, 2) == 2 && rule(512, PR_SCENE_PROJ, false, false, 2) == 16 && rule(512, PR_SCENE_PROJ, false, true, 2, 3) == 2 && rule(512, PR_SCENE_PROJ, false, false, 2, 3) == 3);
        CHECK(rule(512, PR_SCENE_PROJ, false, false, -1, 99) == 20 && rule(512, PR_SCENE_PROJ, false, true, 99) == 20);                       // never beyond the last pass
        CHECK(release_pass_for(0, 0, 0, pr_criteria{ 0.0f, 0.0f, 0 }, PR_SCENE_PROJ, false, true, -1, -1) == 0);
        CHECK(release_pass_for(31468, 512, 27400, pr_criteria{ 0.0f, 0.0f, 2 }, PR_SCENE_PROJ, false, false, -1, -1) == 0);                   // three passes: fewer than the five the rule leaves
    }
    // the bytes a timed pass is accounted: 36 per point on an edge pass, 48 otherwise
    CHECK(icp_span_bytes(0, true) == 0 && icp_span_bytes(1, true) == 36 && icp_span_bytes(1, false) == 48 && icp_span_bytes(27400, true) == 986400 && icp_span_bytes(27400, false) == 1315200);
    CHECK(icp_span_bytes(uint64_t(1) << 40, false) == (uint64_t(48) << 40));
    // pose observability: the information calls' argument checks and pr_info_covariance's body (info_covariance), with nothing written on a refusal
    {
        const float nan = std::nanf(""), inf = INFINITY;
        float c2[6] = { 0, 0, 0.8f, 0.1f, 0, 0.8f }, r2[2] = { 0.05f, 0.1f };
        CHECK(info_center_radius_ok("job_sanitize", c2, r2, 2) == PR_OK && info_center_radius_ok("job_sanitize", nullptr, nullptr, 0) == PR_OK);
        CHECK(info_center_radius_ok("job_sanitize", nullptr, r2, 2) == PR_ERR_INVALID && info_center_radius_ok("job_sanitize", c2, nullptr, 2) == PR_ERR_INVALID);
        for (float bad : { nan, inf, -inf }) { float c[6]; std::memcpy(c, c2, sizeof c); c[5] = bad; CHECK(info_center_radius_ok("job_sanitize", c, r2, 2) == PR_ERR_INVALID); }
        for (float bad : { 0.0f, -0.05f, nan, inf }) { float r[2] = { 0.05f, bad }; CHECK(info_center_radius_ok("job_sanitize", c2, r, 2) == PR_ERR_INVALID); }
        CHECK(info_scene_ok("job_sanitize", PR_SCENE_PROJ, &sp) == PR_OK && info_scene_ok("job_sanitize", PR_SCENE_GRID, &sg) == PR_OK);
        CHECK(info_scene_ok("job_sanitize", PR_SCENE_PROJ, nullptr) == PR_ERR_INVALID && info_scene_ok("job_sanitize", 9, &sp) == PR_ERR_INVALID);
        { pr_scene_grid b = sg; b.rec = nullptr; CHECK(info_scene_ok("job_sanitize", PR_SCENE_GRID, &b) == PR_ERR_INVALID); }
        pr_pose_info pi{}; pr_pose_eig pe{};
        pi.n_points = pi.n_valid = 100; pi.rho = 0.1f; pi.sum_w = 100.0; pi.sum_wr2 = 1.0e-4;
        const double lam[6] = { 0.0, -1.0e-20, 1.0e-9, 1.0e-3, 0.5, 1.0 };
        for (int k = 0; k < 6; ++k) { pe.lambda[k] = lam[k]; pe.V[6 * k + k] = 1.0; }
        double cov[21]; uint32_t rank = 9; double s2 = 9.0;
        for (int i = 0; i < 21; ++i) cov[i] = 7.0;
        auto untouched = [&] { bool same = rank == 9 && s2 == 9.0; for (double v : cov) same = same && v == 7.0; return same; };
        CHECK(info_covariance(nullptr, &pe, 1.0, 0.0, cov, &rank, &s2) == PR_ERR_INVALID && info_covariance(&pi, nullptr, 1.0, 0.0, cov, &rank, &s2) == PR_ERR_INVALID);
        for (double bad : { -1.0e-9, (double)nan, (double)inf }) CHECK(info_covariance(&pi, &pe, 1.0, bad, cov, &rank, &s2) == PR_ERR_INVALID);
        CHECK(info_covariance(&pi, &pe, (double)nan, 0.0, cov, &rank, &s2) == PR_ERR_INVALID);
        { pr_pose_info few = pi; few.n_valid = 6; CHECK(info_covariance(&few, &pe, 0.0, 0.0, cov, &rank, &s2) == PR_ERR_INVALID && info_covariance(&few, &pe, -1.0, 0.0, cov, &rank, &s2) == PR_ERR_INVALID); }
        { pr_pose_info empty = pi; empty.sum_w = 0.0; CHECK(info_covariance(&empty, &pe, 0.0, 0.0, cov, &rank, &s2) == PR_ERR_INVALID); }
        CHECK(untouched());
        CHECK(info_covariance(&pi, &pe, 0.0, 0.0, nullptr, nullptr, nullptr) == PR_OK);
        CHECK(info_covariance(&pi, &pe, 2.0, 1.0e-6, cov, &rank, &s2) == PR_OK && rank == 3 && s2 == 4.0);
        CHECK(cov[0] == 0.0 && cov[6] == 0.0 && cov[11] == 0.0 && cov[15] == 4.0 * (1.0 / 1.0e-3) && cov[18] == 4.0 * (1.0 / 0.5) && cov[20] == 4.0 && cov[1] == 0.0 && cov[19] == 0.0);
        CHECK(info_covariance(&pi, &pe, 0.0, 0.0, cov, &rank, &s2) == PR_OK && rank == 4 && s2 == (1.0e-4 / 100.0) * 100.0 / 94.0);
    }
    // mixed batches.  plan_meshes: 3 meshes, 7 hypotheses, mesh 1 unused -- the groups in mesh order, the order stable within a group
    const pr_mesh_ref m3[3] = { { tris, 5 }, { nullptr, 0 }, { reinterpret_cast<const pr_triangle *>(uintptr_t(0x11000)), 9 } };
    const uint32_t idx7[7] = { 2, 0, 2, 0, 2, 2, 0 }, order7[7] = { 1, 3, 6, 0, 2, 4, 5 };
    {
        MeshPlan pl;
        CHECK(plan_meshes("job_sanitize", m3, 3, idx7, 7, pl) == PR_OK);
        CHECK(pl.mesh.size() == 2 && pl.mesh[0].tris_dev == m3[0].tris_dev && pl.mesh[0].n_tris == 5 && pl.mesh[1].tris_dev == m3[2].tris_dev && pl.mesh[1].n_tris == 9);
        CHECK(pl.start == (std::vector<uint32_t>{ 0, 3, 7 }));
        CHECK(pl.order == std::vector<uint32_t>(order7, order7 + 7));
        CHECK(pl.box == (std::vector<uint32_t>{ 0, 0, 0, 1, 1, 1, 1 }));
        MeshPlan none_planned;                                                                             // no hypotheses, a valid table
        CHECK(plan_meshes("job_sanitize", m3, 3, idx7, 0, none_planned) == PR_OK && none_planned.start == std::vector<uint32_t>{ 0 } && none_planned.order.empty() && none_planned.mesh.empty());
        auto refused_plan = [&](const pr_mesh_ref *t, uint32_t n, const uint32_t *ix, size_t P) { MeshPlan p; CHECK(plan_meshes("job_sanitize", t, n, ix, P, p) == PR_ERR_INVALID); };
        refused_plan(nullptr, 3, idx7, 7);
        refused_plan(m3, 0, idx7, 7);
        refused_plan(m3, 3, nullptr, 7);
        { const pr_mesh_ref bad[3] = { m3[0], { nullptr, 4 }, m3[2] }; refused_plan(bad, 3, idx7, 7); }        // triangles and no array
        { const uint32_t ix[7] = { 2, 0, 2, 3, 2, 2, 0 }; refused_plan(m3, 3, ix, 7); }                      // an index equal to n_meshes
        { const uint32_t ix[7] = { 2, 0, 2, 0, 2, 2, 0xffffffffu }; refused_plan(m3, 3, ix, 7); }
    }
    // Batch on that plan, with tagged records: gather and scatter are inverse, the pyramid's rows land at l * P + caller, the matrix goes back by rows
    // and columns, the inverse is the cover walk's; one mesh: every operation the identity, nothing copied
    {
        struct Rec { uint32_t tag; };
        std::vector<pr_mat4> poses7(7);
        for (uint32_t i = 0; i < 7; ++i) { identity16(poses7[i].m); poses7[i].m[3] = (float)i; }
        Batch b;
        CHECK(b.make("job_sanitize", MeshArg::table(m3, 3, idx7), poses7.data(), 7) == PR_OK);
        CHECK(b.mixed && b.P == 7 && b.src.plan == &b.pl && b.src.tris == nullptr && b.src.n_tris == 0 && b.order() == b.pl.order.data() && b.poses == b.grouped.data());
        for (uint32_t j = 0; j < 7; ++j) CHECK(b.caller(j) == order7[j] && b.poses[j].m[3] == (float)order7[j]);
        std::vector<Rec> x(7), store, back(7, Rec{ 99 });
        for (uint32_t i = 0; i < 7; ++i) x[i].tag = i;
        const Rec *run = b.gather(x.data(), store);
        CHECK(run == store.data() && run != x.data());
        for (uint32_t j = 0; j < 7; ++j) CHECK(run[j].tag == order7[j]);
        b.scatter(run, back.data());
        for (uint32_t i = 0; i < 7; ++i) CHECK(back[i].tag == x[i].tag);                                   // scatter(gather(x)) == x
        b.scatter(run, static_cast<Rec *>(nullptr));                                                        // an output nobody wants
        std::vector<Rec> lv(3 * 7), lv_out(3 * 7, Rec{ 99 });
        for (uint32_t l = 0; l < 3; ++l) for (uint32_t j = 0; j < 7; ++j) lv[l * 7 + j].tag = 100 * l + j;
        b.scatter(lv.data(), lv_out.data(), 3);
        for (uint32_t l = 0; l < 3; ++l) for (uint32_t j = 0; j < 7; ++j) CHECK(lv_out[l * 7 + order7[j]].tag == 100 * l + j);
        std::vector<Rec> mat(49), mat_out(49, Rec{ 99 });
        for (uint32_t k = 0; k < 49; ++k) mat[k].tag = k;
        b.scatter_matrix(mat.data(), mat_out.data());
        for (uint32_t a = 0; a < 7; ++a) for (uint32_t c = 0; c < 7; ++c) CHECK(mat_out[order7[a] * 7 + order7[c]].tag == a * 7 + c);
        const std::vector<uint32_t> where = b.inverse();
        CHECK(where.size() == 7);
        for (uint32_t j = 0; j < 7; ++j) CHECK(where[order7[j]] == j);
        std::vector<Rec> tmp;
        CHECK(b.temp(tmp, 49, back.data()) == tmp.data() && tmp.size() == 49);
        Batch bad;                                                                                          // a refused table leaves the error
        CHECK(bad.make("job_sanitize", MeshArg::table(m3, 0, idx7), poses7.data(), 7) == PR_ERR_INVALID);
        Batch one;
        CHECK(one.make("job_sanitize", MeshArg::one(tris, 5), poses7.data(), 7) == PR_OK);
        CHECK(!one.mixed && one.poses == poses7.data() && one.grouped.empty() && one.src.tris == tris && one.src.n_tris == 5 && one.src.plan == nullptr && one.order() == nullptr);
        for (uint32_t j = 0; j < 7; ++j) CHECK(one.caller(j) == j && one.inverse()[j] == j);
        std::vector<Rec> unused;
        CHECK(one.gather(x.data(), unused) == x.data() && unused.empty());                                  // the caller's pointer, no copy
        CHECK(one.temp(unused, 49, mat.data()) == mat.data() && unused.empty());
        one.scatter(x.data(), x.data()); one.scatter_matrix(mat.data(), mat.data());                        // onto themselves: nothing moves
        for (uint32_t i = 0; i < 7; ++i) CHECK(x[i].tag == i);
        for (uint32_t k = 0; k < 49; ++k) CHECK(mat[k].tag == k);
        one.scatter(lv.data(), lv_out.data(), 3);                                                           // another array: a plain copy
        for (uint32_t k = 0; k < 21; ++k) CHECK(lv_out[k].tag == lv[k].tag);
    }
    // camera_centers against the expression as pr_pose_information and pr_contour_information each wrote it out before they shared it, bit for bit
    {
        auto reference = [](const float *M, const float *cm, int a) {
            const double v = (((double)M[4 * a] * (double)cm[0] + (double)M[4 * a + 1] * (double)cm[1]) + (double)M[4 * a + 2] * (double)cm[2]) + (double)M[4 * a + 3];
            return (float)(v / 1000.0);
        };
        auto same_bits = [](float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; };
        std::vector<pr_mat4> ps(3);
        for (uint32_t i = 0; i < 3; ++i) {                                                                  // rotations about (1, 2, 3) by 0.7 + i rad, translations in mm
            const double th = 0.7 + i, n = std::sqrt(14.0), u[3] = { 1 / n, 2 / n, 3 / n }, c = std::cos(th), s = std::sin(th);
            const double R[9] = { c + u[0] * u[0] * (1 - c), u[0] * u[1] * (1 - c) - u[2] * s, u[0] * u[2] * (1 - c) + u[1] * s,
                                  u[1] * u[0] * (1 - c) + u[2] * s, c + u[1] * u[1] * (1 - c), u[1] * u[2] * (1 - c) - u[0] * s,
                                  u[2] * u[0] * (1 - c) - u[1] * s, u[2] * u[1] * (1 - c) + u[0] * s, c + u[2] * u[2] * (1 - c) };
            identity16(ps[i].m);
            for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) ps[i].m[4 * r + k] = (float)R[3 * r + k]; ps[i].m[4 * r + 3] = 31.7f * (r + 1) - 100.3f * i + 801.9f * (r == 2); }
        }
        const float cm2[6] = { 12.34f, -56.78f, 9.1011f, -3.3f, 44.125f, 70.7f }, rr2[2] = { 0.05f, 0.125f };
        float c[9], rad[3];
        camera_centers(ps.data(), nullptr, 1, cm2, rr2, c, rad);                                             // one pose, one mesh
        for (int a = 0; a < 3; ++a) CHECK(same_bits(c[a], reference(ps[0].m, cm2, a)) && c[a] != 0.0f);
        CHECK(rad[0] == rr2[0]);
        const uint32_t ix[3] = { 1, 0, 1 };
        const pr_mesh_ref m2[2] = { m3[0], m3[2] };
        camera_centers(ps.data(), ix, 3, cm2, rr2, c, rad);                                                  // the caller's order (pr_contour_information_multi)
        for (uint32_t j = 0; j < 3; ++j) {
            for (int a = 0; a < 3; ++a) CHECK(same_bits(c[3 * j + a], reference(ps[j].m, cm2 + 3 * ix[j], a)));
            CHECK(rad[j] == rr2[ix[j]]);
        }
        CHECK(info_center_radius_ok("job_sanitize", c, rad, 3) == PR_OK);
        Batch b;                                                                                            // the plan's order (pr_pose_information_multi)
        CHECK(b.make("job_sanitize", MeshArg::table(m2, 2, ix), ps.data(), 3) == PR_OK && b.pl.order == (std::vector<uint32_t>{ 1, 0, 2 }));
        std::vector<uint32_t> mesh_of;
        camera_centers(b.poses, b.gather(ix, mesh_of), 3, cm2, rr2, c, rad);
        for (uint32_t j = 0; j < 3; ++j) {
            const uint32_t o = b.pl.order[j], m = ix[o];
            for (int a = 0; a < 3; ++a) CHECK(same_bits(c[3 * j + a], reference(ps[o].m, cm2 + 3 * m, a)));
            CHECK(rad[j] == rr2[m]);
        }
        ps[1].m[6] = NAN;                                                                                   // a pose with a NaN entry: a centre the checks refuse
        camera_centers(ps.data(), ix, 3, cm2, rr2, c, rad);
        CHECK(std::isnan(c[3 * 1 + 1]) && same_bits(c[0], reference(ps[0].m, cm2 + 3, 0)) && info_center_radius_ok("job_sanitize", c, rad, 3) == PR_ERR_INVALID);
    }
    // scene caches.  The control words of a kd-tree set at the positions pr_debug_nn_records hands them out at; the fingerprint words of both caches
    {
        using prk::NNInfo;
        const size_t word_of[][2] = { { offsetof(NNInfo, depth), 0 }, { offsetof(NNInfo, rec32_valid), 1 }, { offsetof(NNInfo, qmin), 2 }, { offsetof(NNInfo, qscale), 5 },
                                      { offsetof(NNInfo, wide_state), 8 }, { offsetof(NNInfo, n_wide), 9 }, { offsetof(NNInfo, fp), 12 }, { offsetof(NNInfo, wmin), 16 },
                                      { offsetof(NNInfo, wscale), 19 }, { offsetof(NNInfo, wide_frame_ok), 20 } };
        for (const auto &w : word_of) CHECK(w[0] == 4 * w[1]);
        CHECK(sizeof(NNInfo) == 24 * 4 && offsetof(NNInfo, fp) == 48 && sizeof(NNInfo::qmin) == 12 && sizeof(NNInfo::qscale) == 12 && sizeof(NNInfo::wmin) == 12);
        CHECK(offsetof(prk::FpWords, sample) == 0 && offsetof(prk::FpWords, full) == 8 && offsetof(prk::FpWords, call) == 12 && sizeof(prk::FpWords) == 16);
        CHECK(prk::kWideNone == 0 && prk::kWideValid == 1 && prk::kWideMoreLevels == 2);
        CHECK(sizeof(ProjTail) == 32 && offsetof(ProjTail, exact) == 0 && offsetof(ProjTail, fp) == 4);      // tail words 1..4
        // the packed projective cache: records, two tables, the tail on 16 bytes; carved from a block of that size, every part's last element is inside it
        for (auto [w, h] : { std::pair<size_t, size_t>{ 1, 1 }, { 3, 2 }, { 640, 480 }, { 8192, 2048 } }) {
            const PackedLayout l = packed_layout(w, h);
            const size_t n = w * h, tables = ((w + h) * 4 + 15) / 16 * 16;
            CHECK(l.colf == n * 16 && l.rowf == l.colf + 4 * w && l.tail % 16 == 0 && l.tail == n * 16 + tables && l.tail >= l.rowf + 4 * h && l.bytes == l.tail + 32);
            PackedCache pc;
            pc.rec.p = std::malloc(l.bytes);
            CHECK(pc.rec.p != nullptr);
            if (!pc.rec.p) continue;
            pc.rec.as<float4>()[n - 1] = float4{ 1, 2, 3, 4 }; pc.at<float>(l.colf)[w - 1] = 5.0f; pc.at<float>(l.rowf)[h - 1] = 6.0f;
            ProjTail *t = pc.at<ProjTail>(l.tail);
            *t = ProjTail{ 7u, { 8u, 0u, 9u, 10u }, { 0u, 0u, 0u } };
            CHECK(reinterpret_cast<uintptr_t>(t) % alignof(ProjTail) == 0 && pc.rec.as<float4>()[n - 1].w == 4.0f && pc.at<float>(l.colf)[w - 1] == 5.0f && pc.at<float>(l.rowf)[h - 1] == 6.0f);
            CHECK(pc.at<uint32_t>(l.tail)[0] == 7u && pc.at<uint32_t>(l.tail)[1] == 8u && pc.at<uint32_t>(l.tail)[3] == 9u && pc.at<uint32_t>(l.tail)[4] == 10u);
            std::free(pc.rec.p); pc.rec.p = nullptr;
        }
    }
    // the source arrays of a scene cache, in the order every fingerprint mixes them in: projective pcd, normal; kd-tree pcd, NODES, normal
    {
        const pr_vec3 *pcd = reinterpret_cast<const pr_vec3 *>(uintptr_t(0x20000)), *nrm = reinterpret_cast<const pr_vec3 *>(uintptr_t(0x30000));
        const pr_kdnode *nodes = reinterpret_cast<const pr_kdnode *>(uintptr_t(0x40000));
        pr_scene_proj p32{}; p32.width = 3; p32.height = 2; p32.pcd = pcd; p32.normal = nrm;
        const prk::SceneSources a = prk::scene_sources(p32);
        CHECK(a.p[0] == pcd && a.p[1] == nrm && a.p[2] == nullptr && a.bytes[0] == 72 && a.bytes[1] == 72 && a.bytes[2] == 0);
        CHECK(a.words(0) == reinterpret_cast<const uint32_t *>(pcd) && a.n_words(0) == 18 && a.n_words(1) == 18 && a.n_words(2) == 0 && a.words(2) == nullptr);
        pr_scene_proj big{}; big.width = 8192; big.height = 2048; big.pcd = pcd; big.normal = nrm;
        CHECK(prk::scene_sources(big).bytes[0] == 201326592u && prk::scene_sources(big).n_words(1) == 50331648u);
        pr_scene_nn t{}; t.pcd = pcd; t.normal = nrm; t.nodes = nodes; t.n_points = 11; t.n_nodes = 5;
        const prk::SceneSources b = prk::scene_sources(t);
        CHECK(b.p[0] == pcd && b.p[1] == nodes && b.p[2] == nrm && b.bytes[0] == 132 && b.bytes[1] == 260 && b.bytes[2] == 132);
        CHECK(b.n_words(0) == 33 && b.n_words(1) == 65 && b.n_words(2) == 33);
        pr_scene_nn full{}; full.pcd = pcd; full.normal = nrm; full.nodes = nodes; full.n_points = 0xffffffffu; full.n_nodes = 0xffffffffu;      // no 32-bit product
        CHECK(prk::scene_sources(full).bytes[0] == 12ull * 0xffffffffull && prk::scene_sources(full).bytes[1] == 52ull * 0xffffffffull && prk::scene_sources(full).n_words(1) == 13ull * 0xffffffffull);
        const uint32_t *expected = reinterpret_cast<const uint32_t *>(uintptr_t(0x50000));
        prk::BatchCheck chk{};
        prk::check_sources(chk, b, expected);
        CHECK(chk.fa == a.words(0) && chk.fb == reinterpret_cast<const uint32_t *>(nodes) && chk.fc == a.words(1) && chk.na == 33 && chk.nb == 65 && chk.nc == 33 && chk.fp_expected == expected);
        CHECK(chk.keys == nullptr && chk.flag == nullptr && chk.caller == nullptr);                        // nothing else is touched
        prk::check_sources(chk, a, expected + 1);
        CHECK(chk.fb == a.words(1) && chk.fc == nullptr && chk.na == 18 && chk.nb == 18 && chk.nc == 0 && chk.fp_expected == expected + 1);
    }
    // which set of kd-tree records a scene takes (pick_nn_set): facts = { valid, hit, same arrays, in flight, used }; every rule on a table that the
    // rules behind it would answer differently
    {
        auto pick = [](std::initializer_list<NNSetFacts> f) { return pick_nn_set(f.begin(), (int)f.size()); };
        auto is = [](NNSetPick p, int set, bool hit) { return p.set == set && p.hit == hit; };
        CHECK(is(pick({ { true, false, true, false, 1 }, { true, true, true, false, 9 } }), 1, true));        // 1. a hit -- before a same-arrays set with a lower index
        CHECK(is(pick({ { true, true, true, false, 9 }, { true, true, true, false, 1 } }), 0, true));         //    both hit: the first
        CHECK(is(pick({ { true, false, false, false, 1 }, { true, false, true, true, 9 } }), 1, false));      // 2. valid and of the same arrays, although in flight and used last
        CHECK(is(pick({ { true, false, false, false, 1 }, { false, false, false, false, 2 }, { false, false, true, false, 3 } }), 1, false));      //    (an invalid set's arrays do not count)
        CHECK(is(pick({ { true, false, false, false, 1 }, { false, false, false, true, 9 } }), 1, false));    // 3. the first invalid one
        CHECK(is(pick({ { false, false, false, false, 9 }, { false, false, false, false, 1 } }), 0, false));
        CHECK(is(pick({ { true, false, false, true, 1 }, { true, false, false, false, 9 } }), 1, false));     // 4. least recently used among those no batch reads
        CHECK(is(pick({ { true, false, false, false, 9 }, { true, false, false, false, 1 } }), 1, false));
        CHECK(is(pick({ { true, false, false, false, 1 }, { true, false, false, false, 9 } }), 0, false));
        CHECK(is(pick({ { true, false, false, true, 1 }, { true, false, false, false, 9 }, { true, false, false, false, 5 } }), 2, false));
        CHECK(is(pick({ { true, false, false, true, 9 }, { true, false, false, true, 1 } }), 1, false));      // 5. every set in flight: plain least recently used
        CHECK(is(pick({ { true, false, false, true, 1 }, { true, false, false, true, 9 } }), 0, false));
        CHECK(is(pick({ { true, false, false, true, 4 }, { true, false, false, true, 4 } }), 0, false));
        CHECK(is(pick({ { true, false, false, false, 1 } }), 0, false) && is(pick({ { false, false, false, false, 0 } }), 0, false));
    }
    // how a set is searched (nn_route): the expected values are the parent expressions' results, written out
    {
        auto info_of = [](uint32_t depth, uint32_t rec32_valid = 1, uint32_t wide_state = prk::kWideValid, uint32_t n_wide = 100) {
            prk::NNInfo i{}; i.depth = depth; i.rec32_valid = rec32_valid; i.wide_state = wide_state; i.n_wide = n_wide; i.wide_frame_ok = 1; return i;
        };
        auto is = [](NNRoute r, uint32_t lds, uint32_t stack, bool compact, bool wide) { return r.lds_nodes == lds && r.stack_depth == stack && r.compact == compact && r.wide == wide; };
        // the options' defaults (1024, 0, 1, 1, 1) by depth: 16 entries up to 16, 24 up to 24, the stackless walk beyond
        CHECK(is(nn_route(info_of(0), 5000, 1024, 0, 1, 1, 1), 0, 16, true, true) && is(nn_route(info_of(16), 5000, 1024, 0, 1, 1, 1), 0, 16, true, true));
        CHECK(is(nn_route(info_of(17), 5000, 1024, 0, 1, 1, 1), 0, 24, true, true) && is(nn_route(info_of(24), 5000, 1024, 0, 1, 1, 1), 0, 24, true, true));
        CHECK(is(nn_route(info_of(25), 5000, 1024, 0, 1, 1, 1), 1024, 0, false, false) && is(nn_route(info_of(4096), 5000, 1024, 0, 1, 1, 1), 1024, 0, false, false));
        CHECK(is(nn_route(info_of(10), 5000, 1024, 0, 0, 1, 1), 1024, 0, false, false));                     // nn_stack off: no compact records either
        CHECK(is(nn_route(info_of(10), 5000, 1024, 0, -1, -1, -1), 0, 16, true, true));                      // (the three switches: non-zero is on)
        // compact records invalid; the wide state's three values; no wide nodes; the two options
        CHECK(is(nn_route(info_of(10, 0), 5000, 1024, 0, 1, 1, 1), 0, 16, false, false) && is(nn_route(info_of(10, 2), 5000, 1024, 0, 1, 1, 1), 0, 16, false, false));
        CHECK(is(nn_route(info_of(10, 1, prk::kWideNone), 5000, 1024, 0, 1, 1, 1), 0, 16, true, false) && is(nn_route(info_of(10, 1, prk::kWideMoreLevels), 5000, 1024, 0, 1, 1, 1), 0, 16, true, false));
        CHECK(is(nn_route(info_of(10, 1, prk::kWideValid, 0), 5000, 1024, 0, 1, 1, 1), 0, 16, true, false) && is(nn_route(info_of(10, 1, prk::kWideValid, 1), 5000, 1024, 0, 1, 1, 1), 0, 16, true, true));
        CHECK(is(nn_route(info_of(10), 5000, 1024, 0, 1, 1, 0), 0, 16, true, false) && is(nn_route(info_of(10), 5000, 1024, 0, 1, 0, 1), 0, 16, false, false));
        // stackless: nn_lds_nodes, at most the tree, at most 8192
        CHECK(is(nn_route(info_of(30), 1023, 1024, 0, 1, 1, 1), 1023, 0, false, false) && is(nn_route(info_of(30), 1025, 1024, 0, 1, 1, 1), 1024, 0, false, false));
        CHECK(is(nn_route(info_of(30), 8191, 20000, 0, 1, 1, 1), 8191, 0, false, false) && is(nn_route(info_of(30), 8193, 20000, 0, 1, 1, 1), 8192, 0, false, false));
        CHECK(is(nn_route(info_of(30), 50000, 2147483647, 0, 1, 1, 1), 8192, 0, false, false) && is(nn_route(info_of(30), 50000, -5, 7, 1, 1, 1), 0, 0, false, false));
        CHECK(is(nn_route(info_of(30), 50000, -2147483647 - 1, 7, 0, 1, 1), 0, 0, false, false));
        // stack: nn_lds_records, at most the tree, at most what the stacks and the pass kernel's 512 static bytes leave of 64 KiB -- 504 records beside 16 entries, 248 beside 24
        CHECK(is(nn_route(info_of(16), 5000, 1024, 64, 1, 1, 1), 64, 16, true, true) && is(nn_route(info_of(16), 5000, 1024, -1, 1, 1, 1), 0, 16, true, true));
        CHECK(is(nn_route(info_of(16), 503, 1024, 100000, 1, 1, 1), 503, 16, true, true) && is(nn_route(info_of(16), 505, 1024, 100000, 1, 1, 1), 504, 16, true, true));
        CHECK(is(nn_route(info_of(16), 5000, 1024, 503, 1, 1, 1), 503, 16, true, true) && is(nn_route(info_of(16), 5000, 1024, 512, 1, 1, 1), 504, 16, true, true));
        CHECK(is(nn_route(info_of(24), 247, 1024, 100000, 1, 1, 1), 247, 24, true, true) && is(nn_route(info_of(24), 249, 1024, 2147483647, 1, 1, 1), 248, 24, true, true));
        CHECK(is(nn_route(info_of(24), 5000, 1024, 256, 1, 1, 1), 248, 24, true, true));
        CHECK(16u * 2048u + 504u * 64u + prk::kPassStaticLds == 65536u && 24u * 2048u + 248u * 64u + prk::kPassStaticLds == 65536u);
        // topo_nodes: the stackless count beside any route (the robust pass of a scene without compact records), and what needs no opt-in
        CHECK(nn_route(info_of(16), 5000, 1024, 64, 1, 1, 1).topo_nodes == 1024 && nn_route(info_of(16), 20000, 9000, 64, 1, 0, 1).topo_nodes == 8192 && nn_route(info_of(30), 700, 1024, 64, 1, 1, 1).topo_nodes == 700);
        CHECK(nn_route(info_of(24), 5000, -3, 64, 1, 1, 1).topo_nodes == 0 && nn_route(info_of(30), 50000, 8191, 0, 1, 1, 1).topo_nodes == 8191);
        CHECK(prk::kNNLdsNodesPlain == 4064u && prk::kNNLdsNodesPlain * 16u + prk::kPassStaticLds == 65536u && prk::kNNLdsNodesMax == 8192u);
        CHECK(is(nn_route(info_of(24), 1, 0, 100000, 1, 1, 1), 1, 24, true, true));
    }
    // ---- the frame stages' shared rules and block layouts (frame_stage.h) ----
    {
        const char *fn = "job_sanitize";
        const size_t good[][2] = { { 1, 1 }, { 65535, 1 }, { 1, 65535 }, { 8192, 8192 }, { 65535, 1024 } };
        const size_t bad[][2] = { { 0, 7 }, { 7, 0 }, { 65536, 1 }, { 1, 65536 }, { 65535, 1025 }, { 8193, 8192 } };
        for (const auto &s : good) CHECK(depth_frame_ok(fn, "a frame", s[0], s[1]) == PR_OK);
        for (const auto &s : bad) CHECK(depth_frame_ok(fn, "a frame", s[0], s[1]) == PR_ERR_INVALID);
        CHECK(depth_frame_ok(fn, 1) == PR_OK && depth_frame_ok(fn, (size_t)1 << 26) == PR_OK);
        CHECK(depth_frame_ok(fn, 0) == PR_ERR_INVALID && depth_frame_ok(fn, ((size_t)1 << 26) + 1) == PR_ERR_INVALID);
        // the gate: each limit from both sides
        const uint32_t top = 0x7FFFFFFFu;
        CHECK(gate_ok(fn, "b", 0, 0, 0, 0) == PR_OK && gate_ok(fn, "b", top, top, top, 1000) == PR_OK);
        CHECK(gate_ok(fn, "b", top + 1, 0, 0, 0) == PR_ERR_INVALID && gate_ok(fn, "b", 0, top + 1, 0, 0) == PR_ERR_INVALID && gate_ok(fn, "b", 0, 0, top + 1, 0) == PR_ERR_INVALID);
        CHECK(gate_ok(fn, "b", 500, 500, 0, 0) == PR_OK && gate_ok(fn, "b", 501, 500, 0, 0) == PR_ERR_INVALID && gate_ok(fn, "b", 501, 0, 0, 0) == PR_OK);      // max_mm 0: no upper gate
        CHECK(gate_ok(fn, "b", 0, 0, 0, 1001) == PR_ERR_INVALID);
        // the window: the radius at its limit, a count without a window, the count at (2 r + 1)^2 - 1
        CHECK(window_ok(fn, "b", "r", 0, 2, "c", 0) == PR_OK && window_ok(fn, "b", "r", 2, 2, "c", 0) == PR_OK && window_ok(fn, "b", "r", 3, 2, "c", 0) == PR_ERR_INVALID);
        CHECK(window_ok(fn, "b", "r", 0, 2, "c", 1) == PR_ERR_INVALID && window_ok(fn, "b", "r", 1, 2, "c", 1) == PR_OK);
        CHECK(window_ok(fn, "b", "r", 1, 2, "c", 8) == PR_OK && window_ok(fn, "b", "r", 1, 2, "c", 9) == PR_ERR_INVALID);
        CHECK(window_ok(fn, "b", "r", 2, 2, "c", 24) == PR_OK && window_ok(fn, "b", "r", 2, 2, "c", 25) == PR_ERR_INVALID);
        // the dispatch hands the pointer on unchanged, typed by the flag
        int32_t wide[2] = { 5, 6 };
        CHECK(with_depth(static_cast<const void *>(wide), true, [&](auto *p) { return sizeof *p == 4 && (const void *)p == wide; }));
        CHECK(with_depth(static_cast<void *>(wide), false, [&](auto *p) { return sizeof *p == 2 && (void *)p == wide; }));
        CHECK(depth_bytes(true) == 4 && depth_bytes(false) == 2);
        // a block's parts: each on its alignment, in order, none overlapping, bytes() the end of the last one
        struct Part { size_t at, bytes, align; };
        const auto parts_ok = [&](std::initializer_list<Part> parts, size_t total) {
            size_t end = 0;
            for (const Part &p : parts) { CHECK(p.at % p.align == 0 && p.at >= end && p.at - end < p.align); end = p.at + p.bytes; }
            CHECK(end == total);
        };
        { Block b; CHECK(b.take<uint32_t>(3) == 0 && b.take<uint8_t>(1, 1) == 12 && b.take<uint64_t>(0) == 16 && b.take<uint16_t>(1, 256) == 256 && b.bytes() == 258); }
        { uint32_t words[8] = {}; const ScanRows r(words, 4, 3); CHECK(ScanRows::words(3) == 7 && r.count == words + 1 && r.off == words + 4 && r.total == words + 7); }
        for (uint32_t n_planes : { 1u, (uint32_t)PR_PLANE_MAX_PLANES })
            for (uint32_t rows : { 1u, 8192u })                       // a frame of one row; 8192 rows at stride 1
                for (bool own : { false, true }) {
                    const PlaneBlock l(n_planes, rows, own);
                    parts_ok({ { l.rounds, sizeof(prk::PlaneRound) * n_planes, 16 }, { l.rows, 4 * (2 * (size_t)rows + 1), 16 }, { l.pts, sizeof(prk::PlaneSample) * PR_PLANE_MAX_SAMPLES, 16 },
                               { l.nrm, sizeof(pr_vec3) * PR_PLANE_MAX_SAMPLES, 16 }, { l.support, own ? 4 * (size_t)n_planes * PR_PLANE_MAX_CANDIDATES : 0, 16 } }, l.b.bytes());
                }
        for (uint32_t max_segments : { 1u, (uint32_t)PR_SEGMENT_MAX })
            for (uint32_t n_px : { 1u, 1u << 26 }) {
                const uint32_t n_chunks = (n_px + prk::kSegChunk - 1) / prk::kSegChunk;
                const SegBlock l(max_segments, n_chunks, n_px);
                parts_ok({ { l.ctl, sizeof(prk::SegControl), 16 }, { l.acc, sizeof(segments::Acc) * max_segments, 16 }, { l.rank, 2 * (size_t)PR_SEGMENT_MAX_ROOTS, 16 },
                           { l.roots, sizeof(prk::SegRoot) * PR_SEGMENT_MAX_ROOTS, 16 }, { l.chunks, 4 * (2 * (size_t)n_chunks + 1), 16 }, { l.parent, 4 * (size_t)n_px, 16 },
                           { l.count, 4 * (size_t)n_px, 4 } }, l.b.bytes());
            }
        {
            const SegPinned l;
            parts_ok({ { l.ctl, sizeof(prk::SegControl), 16 }, { l.roots, sizeof(prk::SegRoot) * PR_SEGMENT_MAX_ROOTS, 16 }, { l.rank, 2 * (size_t)PR_SEGMENT_MAX_ROOTS, 16 },
                       { l.acc, sizeof(segments::Acc) * PR_SEGMENT_MAX, 16 } }, l.b.bytes());
            CHECK(l.ctl == 0 && l.roots == sizeof(prk::SegControl));      // the compaction writes the control words and the roots as one run
        }
        for (uint32_t n_models : { 0u, 1u, (uint32_t)PR_PPF_MAX_MODELS })      // 0: pr_ppf_vote's block, without a table
            for (uint32_t n_refs : { 1u, (uint32_t)PR_PPF_MAX_SCENE_POINTS })
                for (uint32_t n_peaks : { 1u, (uint32_t)PR_PPF_MAX_PEAKS }) {
                    const VoteBlock l(n_models, n_refs, n_peaks);
                    const size_t pk = sizeof(pr_ppf_peak) * n_refs * n_peaks * (n_models ? n_models : 1);
                    parts_ok({ { l.models, sizeof(prk::PpfModelRec) * n_models, 16 }, { l.peaks, pk, 16 }, { l.refs, sizeof(prk::PpfRef) * n_refs, 16 } }, l.b.bytes());
                    CHECK(l.back_words() * sizeof(uint32_t) == l.b.bytes() - l.peaks && (l.peaks - l.models) % 16 == 0);
                }
    }
    std::printf("job_sanitize: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
