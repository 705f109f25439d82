// include/flame/params.h -- flame::Params as flame_ros fills it.
//
// Every field below is assigned from a rosparam by the reference frontends (reference
// src/flame_offline_tum.cc:158-249, src/flame_offline_asl.cc, src/flame_nodelet.cc:220-330);
// defaults are the values of cfg/flame_offline_tum.yaml.  The regulariser / triangle-filter fields
// drive the GPU tail; min_grad_mag, detection_win_size, max_dropouts, zparams.win_size and
// zparams.epipolar_line_var drive the GPU feature front end (flame/gpu_frontend.h), and so do this
// build's own switches (zero_mean_matching, gain_invariant_matching, min_epipolar_grad,
// warp_matching_window, carry_features: all off by default); the rest are
// carried so the frontends compile and can be forwarded to another feature pipeline unchanged.
#pragma once

namespace flame {

namespace optimizers {
namespace nltgv2_l1_graph_regularizer {
struct Params {
  float data_factor = 0.15f;  // cfg/flame_offline_tum.yaml:93
  float step_x = 0.001f;      // :94
  float step_q = 125.0f;      // :95
  float theta = 0.25f;        // :96
  float x_min = 0.0f;         // idepth clamp after the prox ([UPSTREAM-RECALL] 0..10)
  float x_max = 10.0f;
};
}  // namespace nltgv2_l1_graph_regularizer
}  // namespace optimizers

struct InverseDepthFilterParams {  // params_.zparams (reference src/flame_offline_tum.cc:224,231)
  int win_size = 5;
  float epipolar_line_var = 4.0f;
};
struct FeatureDetectionParams {  // params_.fparams (:214,225)
  float min_grad_mag = 5.0f;
  int win_size = 5;
};

struct Params {
  // output / display filters (reference src/flame_offline_tum.cc:158-192, yaml :19-57)
  bool debug_quiet = false;
  float scene_color_scale = 1.0f;
  bool do_oblique_triangle_filter = true;
  float oblique_normal_thresh = 1.57f;
  float oblique_idepth_diff_factor = 0.35f;
  float oblique_idepth_diff_abs = 0.1f;
  bool do_edge_length_filter = true;
  float edge_length_thresh = 0.333f;
  bool do_idepth_triangle_filter = true;
  float min_triangle_idepth = 0.01f;
  // debug images (:195-202)
  bool debug_draw_wireframe = true, debug_draw_features = true, debug_draw_detections = false;
  bool debug_draw_matches = false, debug_draw_normals = false, debug_draw_idepthmap = true;
  bool debug_draw_text_overlay = true, debug_flip_images = false;
  // threading (:205-206)
  int omp_num_threads = 4, omp_chunk_size = 1024;
  // (this build's own, not a flame_ros key) host threads of the built-in Delaunay triangulator, the one CPU stage in
  // front of the GPU tail: a persistent pool (flame/utils/delaunay.h); 0 = omp_num_threads.  A host that feeds an
  // MI355X has the cores: 10 k points take 2.3 ms on 4 threads of the old fork-per-level scheme, 0.9 ms on 16 of the pool.
  int triangulate_threads = 16;
  // (this build's own) the built-in triangulation runs on the GPU (flame_hip_delaunay: one wavefront per feature builds the
  // feature's star from exact predicates; same contract as the host triangulator, which stays the choice when false).
  // A registered FrontEnd::triangulate takes precedence over both.
  bool triangulate_on_gpu = true;
  // (this build's own) the stage upstream times as `project_graph`: before the graph sync the previous frame's regularised,
  // validity-filtered mesh, still on the device, is warped into the new camera view and z-buffered (flame_hip_predict), and what
  // it shows at every gated feature becomes the `prediction` the regulariser starts from.  Acts under init_with_prediction,
  // when the front end gave no prediction of its own and the previous update succeeded; update() only (updateGraph() has no
  // pose).  Off by default: with it off every frame starts from the features' own idepths, as before.
  bool project_graph = false;
  // (this build's own) the evaluate stage behind every successful update(): the photometric error of the frame's filtered
  // dense idepth map -- the frame's image warped onto the most recent pose frame before it (flame_hip_photo_error) -- fills
  // the stat keys `total_photo_error` / `avg_photo_error` the reference front ends read (src/flame_offline_tum.cc:391-392,
  // src/utils.cc:138-139) and `photo_pixels`, the number of pixels evaluated.  update() only (updateGraph() has neither image
  // nor pose).  Off by default: with it off update() makes exactly the calls it made before and none of the keys appears.
  bool photo_error = false;
  // (this build's own) the matching cost of flame::GpuFrontEnd's epipolar search (gpu_frontend.h; DESIGN.md 5.3 "Matching cost"):
  // true = zero-mean SSD (flame_hip_frontend_set_cost, FLAME_HIP_FE_COST_ZSSD), which a grey offset between a pose frame and the
  // images tracked against it cannot move -- for cameras with auto-exposure (TUM's Kinect, EuRoC); use zparams.win_size >= 7 with
  // it.  Gain is not removed by this cost; gain_invariant_matching below removes it.  Off by default: with it off the front end makes exactly the calls it made before.  Any other
  // registered FrontEnd gets the field carried and has to honour it itself.
  bool zero_mean_matching = false;
  // (this build's own) true = the gain-invariant matching cost (flame_hip_frontend_set_gain_invariant; DESIGN.md 5.3 "Matching
  // cost"): the residual of the reference window after the best fit ref ~ g cur + b, which neither a gain (an exposure step) nor
  // an offset on the images tracked against a pose frame moves -- bit for bit for a power-of-two gain that clips nowhere, up to
  // the 8-bit rounding of the image otherwise.  While on it overrides zero_mean_matching.  A gain on the pose frame itself is not
  // removed.  Off by default: with it off the front end makes exactly the calls it made before.  Any other registered FrontEnd
  // gets the field carried and has to honour it itself.
  bool gain_invariant_matching = false;
  // (this build's own) the reference-patch gradient gate of flame::GpuFrontEnd's tracker (gpu_frontend.h; DESIGN.md 5.3
  // "Reference-patch gradient"; flame_hip_frontend_set_ref_grad): a feature whose reference window has a root-mean-square grey
  // gradient below this ALONG its epipolar line -- an edge parallel to the line, the aperture problem -- is not searched in that
  // frame and fails like an ambiguous match; `num_fail_ref_patch_grad` counts them.  The scale is min_grad_mag's (5 is a fair
  // choice).  0 = off, the default: with it off the front end makes exactly the calls it made before and the key stays unset.
  // Any other registered FrontEnd gets the field carried and has to honour it itself.
  float min_epipolar_grad = 0.f;
  // (this build's own) true = the warped matching window of flame::GpuFrontEnd's tracker (gpu_frontend.h; DESIGN.md 5.3 "Warped
  // window"; flame_hip_frontend_set_warp): the current image is sampled where the reference window's pixels land under the pose
  // change -- an affine map per feature and frame, taken at the prior -- so that a camera that rolls or changes its distance
  // against the pose frame keeps its features.  A feature whose map is out of range (a stretch above 4, an area scale below 1/16)
  // fails like one outside the image; `num_fail_warp` counts them.  Off by default: with it off the front end makes exactly the
  // calls it made before and the key stays unset.  Any other registered FrontEnd gets the field carried and has to honour it itself.
  bool warp_matching_window = false;
  // (this build's own) true = the hand-over of flame::GpuFrontEnd's tracker (gpu_frontend.h; DESIGN.md 5.3 "Hand-over";
  // flame_hip_frontend_set_carry): when a pose frame takes a slot of the pose-frame ring that is in use, the features of the pose
  // frame it evicts are tracked against the new image once more; those the frame emits at a pixel where a detection could sit are
  // re-anchored in the new pose frame with the emitted inverse depth and variance, the others die behind the frame -- so that a
  // camera that hovers keeps its converged features.  `num_carried` / `num_carry_lost` count them.  Off by default: with it off the
  // front end makes exactly the calls it made before and the keys stay unset.  Any other registered FrontEnd gets the field carried
  // and has to honour it itself.
  bool carry_features = false;
  // features (:209-231)
  // do_letterbox ("Process only middle third of image"): honoured by flame::GpuFrontEnd (gpu_frontend.h; DESIGN.md 5.3 "Gates")
  bool do_letterbox = false;
  float min_grad_mag = 5.0f;
  float min_error = 100.0f;
  int detection_win_size = 16;
  int max_dropouts = 5;
  InverseDepthFilterParams zparams;
  FeatureDetectionParams fparams;
  // regulariser (:234-249, yaml :84-99)
  // do_median_filter / do_lowpass_filter: YAML keys regularization/do_median_filter, do_lowpass_filter
  // (cfg/flame_offline_tum.yaml:85-86) that flame_ros never reads => upstream defaults (off); one
  // Jacobi pass of the graph filter on the regularised idepths (row a9)
  bool do_median_filter = false;
  bool do_lowpass_filter = false;
  bool do_nltgv2 = true;
  bool adaptive_data_weights = false;
  bool rescale_data = false;
  bool init_with_prediction = true;
  float idepth_var_max_graph = 0.01f;
  optimizers::nltgv2_l1_graph_regularizer::Params rparams;
  // min_height / max_height ("height of features that are added to graph", yaml :97-98) and
  // check_sticky_obstacles (:99) gate FEATURES, upstream of the variance gate, in the feature
  // pipeline.  min_height / max_height are honoured by flame::GpuFrontEnd (gpu_frontend.h: the band
  // is on iff min_height > -1e14f or max_height < 1e14f, heights along GpuFrontEnd::setUpAxis;
  // DESIGN.md 5.3 "Gates"); for any other registered FrontEnd they are only carried, and the GPU
  // tail behind the features never reads them.  check_sticky_obstacles is carried and honoured by
  // nobody: the reference does not say what it does.
  float min_height = -1e14f, max_height = 1e14f;
  bool check_sticky_obstacles = false;
  // [UPSTREAM-RECALL] switches (not in the reference; defaults = the build's statement, see
  // include/flame_hip.h flame_hip_sync_params and option "d_sign"): flipped when a state dump of a
  // real robustrobotics/flame build disagrees (tools/pin_upstream/)
  int edge_weight_rule = 0;
  float edge_alpha_gain = 0.0f, edge_beta_gain = 0.0f;
  int edge_d_sign = 1;
  // not in the reference: regulariser iterations per update (an upstream constant that no
  // flame_ros YAML key exposes) and the GPU to run on
  int nltgv2_iterations = 200;
  int hip_device = 0;
};

}  // namespace flame
