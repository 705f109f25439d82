// tools/flame_offline_lite.cc -- a ROS-free miniature of the reference's two offline frontends on the facade:
//   flame_offline_tum (reference src/flame_offline_tum.cc:404-412 construct, :565-601 the per-image loop, :628-635
//                      mesh out, :706-707 stats)           = BASELINE config 1's plumbing
//   flame_offline_asl (reference src/flame_offline_asl.cc:398-407 construct with the dataset's K, :423-435 the loop:
//                      pose as Eigen doubles, CAST TO FLOAT for Sophus::SE3f, colour image rectified by the stream,
//                      src/ros_sensor_streams/asl_rgbd_offline_stream.cc:152-345) = BASELINE config 3's plumbing
// dataset index -> image files -> pixels (include/flame_ros/dataset_streams.h, image_io.h) -> flame::Flame::update()
// with a registered FrontEnd -> idepth mesh + stats per frame.
//
// The feature pipeline (detection, epipolar tracking) plugs in through flame::FrontEnd.  With --gpu-frontend it is the GPU one
// (flame/gpu_frontend.h: image -> GPU tracker -> mesh, the depth image only scores the result).  Without the flag it is a stand-in
// that is deliberately simple and says so: one feature per detection_win_size cell (cfg/flame_offline_tum.yaml:78) where the
// dataset's DEPTH image is valid, idepth = 1 / depth at that pixel (what analysis/pass_in_truth feeds,
// src/flame_offline_tum.cc:577-595).  The kept features are triangulated by the library; everything behind the FrontEnd is the
// product path.
//
//   flame_offline_lite [tum] <index.txt> <frame RDF|FLU|...> fx fy cx cy [iters] [options]
//   flame_offline_lite asl <pose_dir> <rgb_dir> <depth_dir> <world frame RDF|FLU|FRD|RFU> [iters] [options]
//     (K, the distortion coefficients and the depth scale come from the sensor.yaml files, as in the reference)
// -> one line per frame:
//   frame <id> time <t> ok <0|1> feats <n> vtx <n> tris <n> edges <n> coverage <c> cost_smooth <s> cost_data <d> rms_vs_truth <r> update_ms <ms> ...
// --project-graph: Params::project_graph on (every frame's solve starts from the previous mesh warped into its view).
// --photo-error: Params::photo_error on; the frame line ends with `photo_total <sum of grey-level errors> photo_avg <per evaluated
// pixel> photo_pixels <n>` (the frame's filtered map against the last pose frame, every tenth frame here; 0 0 0 before the first).
// --gpu-rectify (asl): the grey image is loaded unrectified and rectified by the library's ingest stage on the GPU
// (flame::GpuFrontEnd::setCamera with the dataset's distortion coefficients, GpuFrontEnd::rectify) instead of on the host; the
// frame lines are the same.  Depth handling is unchanged.
// --gpu-frontend: the features come from a flame::GpuFrontEnd (detection + epipolar tracking on the GPU) instead of the depth
// stand-in; the depth image, where present, is used only for rms_vs_truth.  Pose frames stay (id % 10) == 0; the frame line keeps
// its fields (feats = the features the tracker emitted, also on a frame that failed).  The first frames of a sequence fail --
// nothing has passed the variance gate yet -- so the exit code is 3.  In asl mode together with --gpu-rectify the one GpuFrontEnd
// gets setCamera and takes the raw image: no separate rectify call, no host undistortion.  Not together with --dump.
// --debug-images dir (needs --gpu-frontend): Params::debug_draw_detections / debug_draw_matches on; after every frame
// dir/detections_<id>.ppm and dir/matches_<id>.ppm (binary P6, RGB) from getDebugImageDetections() / getDebugImageMatches().
// --letterbox, --min-height H, --max-height H, --up-axis x,y,z (need --gpu-frontend): the reference's features/do_letterbox and
// regularization/nltgv2/{min_height, max_height} (Params::do_letterbox / min_height / max_height, honoured by flame::GpuFrontEnd:
// features only in the middle third of the rows; tracked features whose world point lies outside the height band along the up
// axis -- default 0,-1,0 -- are held back from the mesh).  With one of them the frame line ends with `held_height <n>
// refused_letterbox <n>`; a band the library refuses ends the run with exit code 5.
// --zero-mean (needs --gpu-frontend): Params::zero_mean_matching -- the tracker matches with the zero-mean SSD
// (flame_hip_frontend_set_cost), which a grey offset between a pose frame and the frames tracked against it cannot move: for
// sequences from auto-exposure cameras.  The frame line ends with `cost_mode 1`.  --win-size N (needs --gpu-frontend):
// Params::zparams.win_size, the matching window (odd, <= 9; the zero-mean cost wants >= 7 on smooth imagery).
// --gain-invariant (needs --gpu-frontend): Params::gain_invariant_matching -- the tracker matches with the gain-invariant cost
// (flame_hip_frontend_set_gain_invariant), which neither an exposure step (a gain) nor an offset on the frames tracked against a
// pose frame moves; it overrides --zero-mean.  The frame line ends with `gain_invariant 1`.
// --min-epipolar-grad G (needs --gpu-frontend): Params::min_epipolar_grad -- the tracker's reference-patch gradient gate
// (flame_hip_frontend_set_ref_grad): a feature whose reference window has a root-mean-square gradient below G along its epipolar
// line is not searched.  The frame line ends with `fail_ref_grad <n>`, the stat key num_fail_ref_patch_grad of the frame.
// --warp-window (needs --gpu-frontend): Params::warp_matching_window -- the tracker samples the current image where the reference
// window's pixels land under the pose change (flame_hip_frontend_set_warp): for cameras that roll or change their distance.  The
// frame line ends with `fail_warp <n>`, the stat key num_fail_warp of the frame.
// --carry-features (needs --gpu-frontend): Params::carry_features -- when a pose frame takes a slot of the pose-frame ring that is in
// use, the features of the pose frame it evicts that the frame still emits move to the new pose frame instead of dying
// (flame_hip_frontend_set_carry): for cameras that hover.  The frame line ends with `carried <n> carry_lost <n>`, the stat keys
// num_carried / num_carry_lost of the frame.  --max-poseframes N (needs --gpu-frontend): the ring's size (1 ... 64, default 16).
// --dump dir: frame_<id>.bin = {int32 V, T; float pos[2V], idepth_mu[V], idepth_var[V]; int32 tris[3T]; float idepth[V]}:
// what went into the regulariser and what came out, for a bit-for-bit comparison with the oracle (tests).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "flame/flame.h"
#include "flame/gpu_frontend.h"
#include "flame_ros/dataset_streams.h"

namespace ds = flame_ros::datasets;

namespace {

ds::Frame parseFrame(const char* s) {
  const char* names[] = {"RDF", "FLU", "FRD", "RDF_IN_FLU", "RDF_IN_FRD", "RFU"};
  for (int k = 0; k < 6; ++k) if (!std::strcmp(s, names[k])) return static_cast<ds::Frame>(k);
  return ds::RDF;
}

struct Lite {
  flame::Params params;  // cfg/flame_offline_tum.yaml defaults (= cfg/flame_offline_asl.yaml's for everything used here)
  std::shared_ptr<flame::Flame> sensor;
  std::vector<float> depth;  // the current frame's depth image in metres (shared with the front end)
  std::vector<float> fmu, fvar;  // the features of the current frame as the front end handed them over
  int W = 0, H = 0;
  std::string dump_dir, debug_dir;
  int failed = 0;
  bool gpu_frontend = false;
  std::unique_ptr<flame::GpuFrontEnd> gpu;  // --gpu-frontend: the feature pipeline
  bool raw_camera = false;                  // ... which takes raw images and rectifies them itself (asl --gpu-rectify)
  float D[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  bool gates = false;  // --letterbox / --min-height / --max-height given
  bool have_up = false;
  float up[3] = {0.f, -1.f, 0.f};
  int gates_error = 0;
  int max_poseframes = 16;  // --max-poseframes: flame::GpuFrontEnd's pose-frame ring

  flame::FrontEnd frontEnd() {
    flame::FrontEnd fe;
    fe.track = [this](const flame::FrameInput&, flame::FeatureSet* fs) {
      const int win = params.detection_win_size, cols = W / win, rows = H / win;
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
          const int u = c * win + win / 2, v = r * win + win / 2;
          const float d = depth.empty() ? 0.f : depth[static_cast<size_t>(v) * W + u];
          if (!(d > 0.f)) continue;  // no depth measurement in this cell: no feature
          fs->vtx.push_back(flame::Point2f(static_cast<float>(u), static_cast<float>(v)));
          fs->idepth_mu.push_back(1.0f / d);
          fs->idepth_var.push_back(1e-4f);
        }
      fmu = fs->idepth_mu; fvar = fs->idepth_var;
      return !fs->vtx.empty();
    };
    // (no fe.triangulate: the facade's built-in Delaunay triangulator, flame/utils/delaunay.h)
    return fe;
  }

  void construct(float fx, float fy, float cx, float cy) {
    flame::Matrix3f K, Kinv;
    K(0, 0) = fx; K(0, 1) = 0.f; K(0, 2) = cx; K(1, 0) = 0.f; K(1, 1) = fy; K(1, 2) = cy; K(2, 0) = 0.f; K(2, 1) = 0.f; K(2, 2) = 1.f;
    Kinv(0, 0) = 1.f / fx; Kinv(0, 1) = 0.f; Kinv(0, 2) = -cx / fx; Kinv(1, 0) = 0.f; Kinv(1, 1) = 1.f / fy; Kinv(1, 2) = -cy / fy;
    Kinv(2, 0) = 0.f; Kinv(2, 1) = 0.f; Kinv(2, 2) = 1.f;
    sensor = std::make_shared<flame::Flame>(W, H, K, Kinv, params);
    if (gpu_frontend) {
      gpu.reset(new flame::GpuFrontEnd(W, H, K, params, 4096, max_poseframes));
      if (raw_camera && !gpu->setCamera(W, H, 1, D)) std::fprintf(stderr, "--gpu-rectify: hip_error %d\n", gpu->lastError());
      if (gates && gpu->handle()) {  // (Params carried the band into the constructor; the up axis is the front end's own)
        gates_error = gpu->gates().letterbox || gpu->gates().height_gate ? gpu->lastError() : 0;
        if (!gates_error && have_up && !gpu->setUpAxis(up[0], up[1], up[2])) gates_error = gpu->lastError();
        if (gates_error) std::fprintf(stderr, "gates: hip_error %d\n", gates_error);
      }
      sensor->setFrontEnd(gpu->frontEnd());
    } else {
      sensor->setFrontEnd(frontEnd());
    }
  }

  static void writePpm(const std::string& path, const flame::Image3b& bgr) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return; }
    std::fprintf(f, "P6\n%d %d\n255\n", bgr.cols, bgr.rows);
    std::vector<uint8_t> row(3 * static_cast<size_t>(bgr.cols));
    for (int y = 0; y < bgr.rows; ++y) {
      for (int x = 0; x < bgr.cols; ++x)
        for (int c = 0; c < 3; ++c) row[3 * static_cast<size_t>(x) + c] = bgr(y, x)[2 - c];
      std::fwrite(row.data(), 1, row.size(), f);
    }
    std::fclose(f);
  }

  // one frame: pose in DOUBLE precision as the dataset streams deliver it, cast to float where the reference
  // builds its Sophus::SE3f (src/flame_offline_asl.cc:431, src/flame_offline_tum.cc:566-572)
  void frame(uint32_t id, double time, const ds::Pose& pose_optical, const std::vector<uint8_t>& gray) {
    flame::Image1b img(H, W);
    std::memcpy(static_cast<void*>(&img(0, 0)), gray.data(), gray.size());
    flame::SE3f pose;
    pose.q[0] = static_cast<float>(pose_optical.q.x); pose.q[1] = static_cast<float>(pose_optical.q.y);
    pose.q[2] = static_cast<float>(pose_optical.q.z); pose.q[3] = static_cast<float>(pose_optical.q.w);
    for (int k = 0; k < 3; ++k) pose.t[k] = static_cast<float>(pose_optical.t[k]);
    const bool ok = sensor->update(time, id, pose, img, (id % 10) == 0);
    if (!ok) ++failed;
    std::vector<flame::Point2f> vtx;
    std::vector<float> idepths;
    std::vector<flame::Vector3f> normals;
    std::vector<flame::Triangle> tris;
    std::vector<bool> valid;
    std::vector<flame::Edge> edges;
    sensor->getInverseDepthMesh(&vtx, &idepths, &normals, &tris, &valid, &edges);
    double se = 0.0;
    size_t n = 0;
    for (size_t v = 0; ok && !depth.empty() && v < vtx.size(); ++v) {
      const float d = depth[static_cast<size_t>(vtx[v].y) * W + static_cast<size_t>(vtx[v].x)];
      if (d > 0.f) { const double e = idepths[v] - 1.0 / d; se += e * e; ++n; }
    }
    if (ok && !dump_dir.empty() && fmu.size() == vtx.size()) {  // (every feature passes the variance gate here)
      const std::string path = dump_dir + "/frame_" + std::to_string(id) + ".bin";
      if (FILE* f = std::fopen(path.c_str(), "wb")) {
        const int32_t hdr[2] = {static_cast<int32_t>(vtx.size()), static_cast<int32_t>(tris.size())};
        std::fwrite(hdr, sizeof(hdr), 1, f);
        for (size_t v = 0; v < vtx.size(); ++v) { const float p[2] = {vtx[v].x, vtx[v].y}; std::fwrite(p, sizeof(p), 1, f); }
        std::fwrite(fmu.data(), sizeof(float), fmu.size(), f);
        std::fwrite(fvar.data(), sizeof(float), fvar.size(), f);
        for (size_t t = 0; t < tris.size(); ++t) { const int32_t q[3] = {tris[t][0], tris[t][1], tris[t][2]}; std::fwrite(q, sizeof(q), 1, f); }
        std::fwrite(idepths.data(), sizeof(float), idepths.size(), f);
        std::fclose(f);
      }
    }
    const flame::utils::StatsTracker& st = sensor->stats();
    int feats = static_cast<int>(st.stats("num_feats"));
    if (gpu) {  // what the tracker emitted for THIS frame (num_feats is the last committed frame's)
      int64_t emitted = 0;
      if (gpu->handle() && flame_hip_frontend_info(gpu->handle(), "emitted", &emitted) == 0) feats = static_cast<int>(emitted);
      else feats = 0;
    }
    if (!debug_dir.empty()) {
      writePpm(debug_dir + "/detections_" + std::to_string(id) + ".ppm", sensor->getDebugImageDetections());
      writePpm(debug_dir + "/matches_" + std::to_string(id) + ".ppm", sensor->getDebugImageMatches());
    }
    std::printf("frame %u time %.6f ok %d feats %d vtx %zu tris %zu edges %zu coverage %.4f cost_smooth %.6g cost_data %.6g rms_vs_truth %.6g update_ms %.3f hip_error %d persist_used %d pose_t %.9g %.9g %.9g pose_q %.9g %.9g %.9g %.9g",
                id, time, ok ? 1 : 0, feats, vtx.size(), tris.size(), edges.size(),
                st.stats("coverage"), st.stats("nltgv2_total_smoothness_cost"), st.stats("nltgv2_total_data_cost"),
                n ? std::sqrt(se / n) : 0.0, st.timings("update"), static_cast<int>(st.stats("hip_error")),
                static_cast<int>(st.stats("persist_used")), pose.t[0], pose.t[1], pose.t[2], pose.q[0], pose.q[1], pose.q[2], pose.q[3]);
    if (params.photo_error)  // (appended at the end: without the flag the line is what it was)
      std::printf(" photo_total %.6f photo_avg %.6f photo_pixels %d", st.stats("total_photo_error"), st.stats("avg_photo_error"),
                  static_cast<int>(st.stats("photo_pixels")));
    if (gates) {  // (appended at the end: without the flags the line is what it was)
      int64_t held = 0, refused = 0;
      if (gpu && gpu->handle()) {
        flame_hip_frontend_info(gpu->handle(), "held_height", &held);
        flame_hip_frontend_info(gpu->handle(), "refused_letterbox", &refused);
      }
      std::printf(" held_height %d refused_letterbox %d", static_cast<int>(held), static_cast<int>(refused));
    }
    if (params.zero_mean_matching) {  // (appended at the end: without the flag the line is what it was)
      int64_t mode = -1;
      if (gpu && gpu->handle()) flame_hip_frontend_info(gpu->handle(), "cost_mode", &mode);
      std::printf(" cost_mode %d", static_cast<int>(mode));
    }
    if (params.min_epipolar_grad != 0.f)  // (appended at the end: without the flag the line is what it was)
      std::printf(" fail_ref_grad %d", st.stats().count("num_fail_ref_patch_grad") ? static_cast<int>(st.stats("num_fail_ref_patch_grad")) : -1);
    if (params.gain_invariant_matching) {  // (appended at the end: without the flag the line is what it was)
      int64_t on = -1;
      if (gpu && gpu->handle()) flame_hip_frontend_info(gpu->handle(), "gain_invariant", &on);
      std::printf(" gain_invariant %d", static_cast<int>(on));
    }
    if (params.warp_matching_window)  // (appended at the end: without the flag the line is what it was)
      std::printf(" fail_warp %d", st.stats().count("num_fail_warp") ? static_cast<int>(st.stats("num_fail_warp")) : -1);
    if (params.carry_features)  // (appended at the end: without the flag the line is what it was)
      std::printf(" carried %d carry_lost %d", st.stats().count("num_carried") ? static_cast<int>(st.stats("num_carried")) : -1,
                  st.stats().count("num_carry_lost") ? static_cast<int>(st.stats("num_carry_lost")) : -1);
    std::printf("\n");
  }
};

}  // namespace

int main(int argc, char** argv) {
  std::vector<char*> args;
  Lite L;
  bool gpu_rectify = false, bad_up = false, win_flag = false, rg_flag = false, ring_flag = false;
  for (int k = 1; k < argc; ++k) {
    if (!std::strcmp(argv[k], "--dump") && k + 1 < argc) L.dump_dir = argv[++k];
    else if (!std::strcmp(argv[k], "--project-graph")) L.params.project_graph = true;  // warm-start every frame from the last mesh
    else if (!std::strcmp(argv[k], "--photo-error")) L.params.photo_error = true;      // the evaluate stage behind every frame
    else if (!std::strcmp(argv[k], "--gpu-rectify")) gpu_rectify = true;               // (asl) undistort on the GPU
    else if (!std::strcmp(argv[k], "--gpu-frontend")) L.gpu_frontend = true;           // features from flame::GpuFrontEnd
    else if (!std::strcmp(argv[k], "--debug-images") && k + 1 < argc) L.debug_dir = argv[++k];
    else if (!std::strcmp(argv[k], "--zero-mean")) L.params.zero_mean_matching = true;
    else if (!std::strcmp(argv[k], "--gain-invariant")) L.params.gain_invariant_matching = true;
    else if (!std::strcmp(argv[k], "--warp-window")) L.params.warp_matching_window = true;
    else if (!std::strcmp(argv[k], "--carry-features")) L.params.carry_features = true;
    else if (!std::strcmp(argv[k], "--max-poseframes") && k + 1 < argc) { L.max_poseframes = std::atoi(argv[++k]); ring_flag = true; }
    else if (!std::strcmp(argv[k], "--win-size") && k + 1 < argc) { L.params.zparams.win_size = std::atoi(argv[++k]); win_flag = true; }
    else if (!std::strcmp(argv[k], "--min-epipolar-grad") && k + 1 < argc) { L.params.min_epipolar_grad = static_cast<float>(std::atof(argv[++k])); rg_flag = true; }
    else if (!std::strcmp(argv[k], "--letterbox")) { L.params.do_letterbox = true; L.gates = true; }
    else if (!std::strcmp(argv[k], "--min-height") && k + 1 < argc) { L.params.min_height = static_cast<float>(std::atof(argv[++k])); L.gates = true; }
    else if (!std::strcmp(argv[k], "--max-height") && k + 1 < argc) { L.params.max_height = static_cast<float>(std::atof(argv[++k])); L.gates = true; }
    else if (!std::strcmp(argv[k], "--up-axis") && k + 1 < argc) {
      L.have_up = std::sscanf(argv[++k], "%f,%f,%f", &L.up[0], &L.up[1], &L.up[2]) == 3;
      if (!L.have_up) bad_up = true;
    }
    else args.push_back(argv[k]);
  }
  const bool asl = !args.empty() && !std::strcmp(args[0], "asl");
  if (!args.empty() && (!std::strcmp(args[0], "tum") || asl)) args.erase(args.begin());
  const bool bad_flags = (!L.debug_dir.empty() && !L.gpu_frontend) || (!L.dump_dir.empty() && L.gpu_frontend) ||
                         ((L.gates || L.have_up || L.params.zero_mean_matching || L.params.gain_invariant_matching || L.params.warp_matching_window || L.params.carry_features || win_flag || rg_flag || ring_flag) && !L.gpu_frontend) || bad_up ||
                         (ring_flag && (L.max_poseframes < 1 || L.max_poseframes > 64));
  if (bad_flags || (asl && args.size() < 4) || (!asl && args.size() < 6)) {
    std::fprintf(stderr, "usage: %s [tum] index.txt frame fx fy cx cy [iters] [--dump dir] [--project-graph] [--photo-error] [--gpu-frontend [--debug-images dir]]\n       %s asl pose_dir rgb_dir depth_dir world_frame [iters] [--dump dir] [--project-graph] [--photo-error] [--gpu-rectify] [--gpu-frontend [--debug-images dir]]\n"
                 "  --gpu-frontend: features from the GPU tracker (not with --dump); --debug-images dir: detections_<id>.ppm / matches_<id>.ppm per frame (needs --gpu-frontend)\n"
                 "  --letterbox, --min-height H, --max-height H, --up-axis x,y,z (need --gpu-frontend): features only in the middle third of the rows / only inside the height band along the up axis (default 0,-1,0)\n"
                 "  --zero-mean (needs --gpu-frontend): match with the zero-mean SSD, which a grey offset between frames cannot move (auto-exposure cameras); --win-size N: the matching window (odd, <= 9)\n"
                 "  --gain-invariant (needs --gpu-frontend): match with the gain-invariant cost, which an exposure step between frames cannot move; overrides --zero-mean\n"
                 "  --warp-window (needs --gpu-frontend): sample the current image where the reference window lands under the pose change (cameras that roll or change their distance)\n"
                 "  --carry-features (needs --gpu-frontend): features of a pose frame that the ring evicts move to the pose frame that takes its slot (cameras that hover); --max-poseframes N: the ring's size (1 ... 64, default 16)\n"
                 "  --min-epipolar-grad G (needs --gpu-frontend): do not search a feature whose reference window has a gradient below G along its epipolar line (0 = off)\n",
                 argv[0], argv[0]);
    return 2;
  }
  if (!L.debug_dir.empty()) L.params.debug_draw_detections = L.params.debug_draw_matches = true;
  std::string err;
  if (asl) {
    // ---- flame_offline_asl: K / D / depth scale from the sensor.yaml files, colour image rectified, depth not ----
    ds::AslDataset data(args[0], args[1], std::strcmp(args[2], "-") ? args[2] : "", parseFrame(args[3]));
    if (!data.ok() || data.size() == 0) { std::fprintf(stderr, "cannot read the ASL folders\n"); return 3; }
    if (args.size() > 4) L.params.nltgv2_iterations = std::atoi(args[4]);
    flame_ros::images::PlumbBob cam;
    cam.fx = static_cast<float>(data.K()[0]); cam.fy = static_cast<float>(data.K()[4]);
    cam.cx = static_cast<float>(data.K()[2]); cam.cy = static_cast<float>(data.K()[5]);
    cam.k1 = static_cast<float>(data.D()[0]); cam.k2 = static_cast<float>(data.D()[1]);
    cam.p1 = static_cast<float>(data.D()[2]); cam.p2 = static_cast<float>(data.D()[3]); cam.k3 = static_cast<float>(data.D()[4]);
    const bool distorted = cam.k1 != 0.f || cam.k2 != 0.f || cam.p1 != 0.f || cam.p2 != 0.f || cam.k3 != 0.f;
    if (gpu_rectify && L.gpu_frontend) {  // the one GpuFrontEnd takes the raw image (construct(): setCamera)
      L.raw_camera = true;
      const float D[5] = {cam.k1, cam.k2, cam.p1, cam.p2, cam.k3};
      std::memcpy(L.D, D, sizeof(D));
    }
    uint32_t id = 0;
    ds::AslFrame fr;
    std::unique_ptr<flame::GpuFrontEnd> ingest;  // --gpu-rectify: the library's ingest stage instead of image_io.h undistort()
    while (data.get(&id, &fr)) {
      std::vector<uint8_t> gray;
      if (!ds::loadFramePixels(fr.rgb_file, fr.has_depth ? fr.depth_file : std::string(), static_cast<float>(data.depthScaleFactor()),
                               (distorted && !gpu_rectify) ? &cam : nullptr, false, &L.W, &L.H, &gray, &L.depth, &err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 4;
      }
      if (L.W != data.width() || L.H != data.height()) { std::fprintf(stderr, "image size differs from sensor.yaml's resolution\n"); return 4; }
      if (gpu_rectify && !L.gpu_frontend) {
        if (!ingest) {
          flame::Matrix3f K;
          for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K(r, c) = (r == c) ? 1.f : 0.f;
          K(0, 0) = cam.fx; K(1, 1) = cam.fy; K(0, 2) = cam.cx; K(1, 2) = cam.cy;
          const float D[5] = {cam.k1, cam.k2, cam.p1, cam.p2, cam.k3};
          ingest.reset(new flame::GpuFrontEnd(L.W, L.H, K, L.params, 1, 1));
          if (!ingest->setCamera(L.W, L.H, 1, D)) { std::fprintf(stderr, "--gpu-rectify: hip_error %d\n", ingest->lastError()); return 5; }
        }
        flame::Image1b raw(L.H, L.W), rect(L.H, L.W);
        for (int y = 0; y < L.H; ++y) std::memcpy(raw.ptr<uint8_t>(y), gray.data() + static_cast<size_t>(y) * L.W, L.W);
        if (!ingest->rectify(raw, &rect)) { std::fprintf(stderr, "--gpu-rectify: hip_error %d\n", ingest->lastError()); return 5; }
        for (int y = 0; y < L.H; ++y) std::memcpy(gray.data() + static_cast<size_t>(y) * L.W, rect.ptr<uint8_t>(y), L.W);
      }
      if (!L.sensor) L.construct(cam.fx, cam.fy, cam.cx, cam.cy);
      if (L.gates_error) return 5;
      L.frame(id, fr.time, fr.pose_optical, gray);
    }
  } else {
    // ---- flame_offline_tum ----
    const float fx = std::atof(args[2]), fy = std::atof(args[3]), cx = std::atof(args[4]), cy = std::atof(args[5]);
    ds::TumIndex index(args[0], parseFrame(args[1]));
    if (index.size() == 0) return 3;
    if (args.size() > 6) L.params.nltgv2_iterations = std::atoi(args[6]);
    uint32_t id = 0;
    ds::TumFrame fr;
    while (index.get(&id, &fr)) {
      std::vector<uint8_t> gray;
      if (!ds::loadFramePixels(fr.rgb_file, fr.has_depth ? fr.depth_file : std::string(), index.depthScaleFactor(), nullptr,
                               false, &L.W, &L.H, &gray, &L.depth, &err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 4;
      }
      if (!L.sensor) L.construct(fx, fy, cx, cy);
      if (L.gates_error) return 5;
      L.frame(id, fr.time, fr.pose_optical, gray);
    }
  }
  return L.failed ? 3 : 0;
}
