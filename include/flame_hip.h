/*
 * include/flame_hip.h -- C ABI of libflame_hip.so: FLaME's NLTGV2-L1 graph regulariser and
 * per-triangle stage as hand-written HIP kernels for MI355X (gfx950), and the feature front end in
 * front of them (detection + epipolar inverse-depth tracking, the flame_hip_frontend entry points below).
 *
 * This is the drop-in boundary.  Upstream, flame::Flame::update() (called at reference
 * src/flame_offline_tum.cc:578-579,593-594, src/flame_offline_asl.cc:520,535,
 * src/flame_nodelet.cc:634-635) runs N x optimizers::nltgv2_l1_graph_regularizer::step() on the
 * Delaunay vertex graph and then the per-triangle stage whose results leave through
 * getInverseDepthMesh() (src/flame_offline_tum.cc:628-635).  A maintainer replaces that inner
 * loop by the calls below (INTEGRATION.md shows the binding); the C++ facade in include/flame/
 * does exactly that.
 *
 * Conventions: return 0 = ok, negative = error (flame_hip_strerror()); no exceptions, no global
 * state.  All pointers are HOST pointers owned by the caller for the duration of the call unless
 * the name says _dev.  One handle is not thread-safe; distinct handles are.  Edge e is oriented
 * edges[2e] -> edges[2e+1]; the orientation matters (the source vertex's plane slopes enter K1).
 * All arithmetic is float32 and bit-reproducible: identical inputs give identical bits on every
 * solver path and partitioning (see DESIGN.md "Arithmetic contract").
 */
#ifndef FLAME_HIP_H_
#define FLAME_HIP_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* flame::Params::rparams as loaded at reference src/flame_offline_tum.cc:242-245
 * (defaults cfg/flame_offline_tum.yaml:93-96) + the idepth clamp applied after the prox. */
typedef struct {
  float data_factor; /* lambda  (regularization/nltgv2/data_factor) */
  float step_x;      /* tau     (.../step_x) */
  float step_q;      /* sigma   (.../step_q) */
  float theta;       /* extra-gradient weight (.../theta) */
  float x_min, x_max;
} flame_hip_params;

/* Triangle filter parameters as loaded at reference src/flame_offline_tum.cc:168-192
 * (cfg/flame_offline_tum.yaml:38-53). */
typedef struct {
  int32_t do_oblique_triangle_filter;
  float oblique_normal_thresh;      /* rad */
  float oblique_idepth_diff_factor; /* relative max/min idepth difference */
  float oblique_idepth_diff_abs;    /* absolute max/min idepth difference */
  int32_t do_edge_length_filter;
  float edge_length_thresh; /* fraction of image width */
  int32_t do_idepth_triangle_filter;
  float min_triangle_idepth;
  int32_t width, height;
} flame_hip_tri_params;

typedef struct flame_hip_graph flame_hip_graph; /* opaque; owns device buffers */

enum {
  FLAME_HIP_OK = 0,
  FLAME_HIP_ERR_ARG = -1,     /* bad argument (NULL, negative size, index out of range) */
  FLAME_HIP_ERR_STATE = -2,   /* call order (e.g. solve before upload) */
  FLAME_HIP_ERR_NAN = -3,     /* non-finite input */
  FLAME_HIP_ERR_ALLOC = -4,   /* host or device allocation failed */
  FLAME_HIP_ERR_NODEVICE = -5,
  FLAME_HIP_ERR_NORCCL = -6,  /* librccl.so could not be loaded (flame_hip_comm_* / flame_hip_part_*) */
  FLAME_HIP_ERR_HIP = -1000,  /* -(1000 + hipError_t) */
  FLAME_HIP_ERR_RCCL = -3000  /* -(3000 + ncclResult_t) */
};

/* Solver paths (flame_hip_set_option key "path"). */
enum {
  FLAME_HIP_PATH_AUTO = 0,
  FLAME_HIP_PATH_GLOBAL = 1, /* two kernels per iteration over global arrays */
  FLAME_HIP_PATH_TILE = 2    /* LDS-resident tiles, several iterations per launch */
};

/* Replaces: construction of the regulariser graph inside Flame::update. */
int flame_hip_graph_create(flame_hip_graph** out, int device, int32_t V, int32_t E, int32_t T);
void flame_hip_graph_destroy(flame_hip_graph* g);

/* One handle serves a frame STREAM: every frame of FLaME is a new graph (reference
 * src/flame_offline_tum.cc:578: update() re-triangulates per image).  Sets the sizes of the NEXT
 * flame_hip_graph_upload*; the handle keeps its stream, events, device buffers (capacity), host
 * plan buffers and the tile cost-density grid.  Registered halo lists are dropped.  Waits for any
 * solve still in flight. */
int flame_hip_graph_resize(flame_hip_graph* g, int32_t V, int32_t E, int32_t T);

/* Options are set BEFORE upload.  Keys: "path" (enum above), "tile_own" (target own vertices
 * per tile), "tile_depth" (halo depth = iterations per launch), "tile_threads", "use_graph"
 * (replay launches from a hipGraph), "plan_device" (1 = build halo-tile plans on the GPU, default),
 * "plan_reuse" (1 = default: on a frame stream the device builder takes the PARTITION of a frame from
 * the previous frame's tile map while the frames hold about as many vertices, instead of sorting and
 * bisecting again; results do not depend on the partition; flame_hip_get_info "plan_reused"),
 * "plan_mini" (1 = default: a graph sync of a small frame -- up to 2048 vertices / 4096 triangles, a
 * reused partition, a predicted edge count -- derives the edges and builds everything in front of the
 * tile pass in ONE launch of one workgroup instead of two dozen dependent ones; flame_hip_get_info
 * "plan_mini" tells whether the current plan was made that way),
 * (flame_hip_get_info "tile_imbalance_pct": 100 x max / mean of the tiles' modelled cost, local edges + 2 x
 * local vertices -- a launch lasts as long as its slowest tile; 125-155 on 50 k-vertex frames, the border
 * tiles' long hull edges)
 * "tile_single_max" (auto: graphs up to this many vertices become ONE LDS-resident tile, default
 * 512, up to 2048; a graph whose tile does not fit after all is partitioned, and the handle stops
 * trying at that size: flame_hip_get_info "single_cap"), "stream_depth" (0 = off, default; > 0: halo
 * depth of graphs of up to 2048 vertices in place of the automatic 8 -- for handles that solve every
 * graph ONCE, where the plan of shallow tiles is cheaper than the launches deep tiles save), "persist"
 * (default 1: a graph of 2 .. 256 halo tiles -- at most one per CU -- is solved by ONE launch of RESIDENT tiles:
 * neighbours hand their results over through uncached, round-tagged copies of the state arrays every `depth`
 * iterations instead of meeting at a kernel boundary; same bits, any placement of the tiles on the chip; 0: one
 * launch per `depth` iterations; flame_hip_get_info "persist_used" tells whether the last solve ran that way.  r05: with
 * automatic tile sizes that covers every graph up to ~240 000 vertices -- beyond 256 x 196 the tiles grow FAT (one per CU,
 * shallower halos, 12-byte incidence slots where 16 do not fit the LDS: flame_hip_get_info "tile_fat", "tile_slot12"); a handle
 * with "persist" 0 keeps the partition of two rounds of smaller tiles there.  The
 * launch ASSUMES that all its workgroups are on the chip at once.  The library keeps the tile count within the
 * CU count and lets one handle per device and process run such a launch at a time (another handle solving at the
 * same moment uses ordinary launches), but a foreign kernel that holds CUs for long -- another process, another
 * library -- can still keep tiles from starting: every wait inside the launch is bounded (4 ms until the handle has measured
 * a round of the current graph, then max(0.5 ms, 8 x that round); option "persist_timeout_us" > 0 fixes it; flame_hip_get_info
 * "persist_timeout_us" = what the last launch was given), a launch that
 * gave up is noticed at the next synchronising call and REPEATED by ordinary launches from its untouched source
 * buffers ("persist_recovered" counts those; r05: SEVERAL solves queued without a synchronising call between them are
 * repeated as a whole -- the error word does not say which one gave up, so the source of the first is copied aside when
 * the second is queued and every solve since is logged; FLAME_HIP_ERR_STATE only when something other than solves wrote
 * the state in between), and the whole process then stays off resident tiles for 16 solves, doubling with every further
 * give-up ("persist_gave_up").  How far the tiles of a handle's last give-up got, read from the hand-off copies afterwards:
 * "persist_gave_up_tile" / "_round" = the tile that had handed over the fewest rounds (0: it never started; otherwise it is the
 * late one or stood next to it) and how many, "_front_round" the most any tile had, "_not_started" tiles that had handed over
 * none, "_rounds" / "_tiles" / "_one_xcd" / "_timeout_us" the launch's own numbers; "persist_backoff" = solves the device's lease still
 * sits out (plans uploaded meanwhile are sized for launches), "one_xcd_allowed" = 0 once a one-XCD launch has given up.  "one_xcd" (r06, default 1): a graph of up to 32 resident tiles -- automatic sizes give 32 tiles to
 * graphs of 770 .. 1 280 vertices -- keeps them on ONE XCD (the launch has 8 x ntiles workgroups, every 8th carries a tile) and hands
 * over through ordinary memory, i.e. that XCD's L2, instead of uncached memory: 1.2 k vertices 0.89 -> 0.82 us per iteration.  Which
 * XCD a workgroup lands on is the dispatcher's habit, not a guarantee; the round tags and the bounded polls keep the result right
 * regardless: tiles that cannot see each other time out, the solve is repeated by launches and the device's lease drops the mode for
 * the rest of the process (flame_hip_get_info "one_xcd_used").  Tuning: "poll_delay" (x 256 clocks between a round's stores and its first poll pass, -1 =
 * automatic), "need_marks" (1 = default: fat tiles hand over only the entries somebody polls).  Diagnostics: "plan_timing" (1-5:
 * the plan builders print their stages' times to stderr); with option "persist_prof" = <tile + 1>
 * "persist_prof_0".."persist_prof_3" return that tile's time split of the last solve's rounds in 10 ns ticks:
 * iterations + stores, poll of the halo entries, halo applied + barrier, and the number of rounds),
 * "lane_order" (lanes of the tile plan re-assigned against LDS bank conflicts:
 * 0 never, 1 = when an uploaded graph is solved a second time (default; a frame stream never pays),
 * 2 = while the plan is built), "balance", "order_mode", "host_threads", "lds_bytes", "profile",
 * "d_sign" ([UPSTREAM-RECALL] switch: +1 (default) the edge vector entering K1 is d = pos_i - pos_j,
 * -1 it is pos_j - pos_i).  Unknown key -> FLAME_HIP_ERR_ARG.  The library reads NO environment variable: everything that
 * changes its behaviour is an option of a handle (fault injection for the tests exists only in a library of its own,
 * libflame_hip_hooks.so, flame_ros_amd/build.py). */
int flame_hip_set_option(flame_hip_graph* g, const char* key, int32_t value);
int flame_hip_get_info(const flame_hip_graph* g, const char* key, int64_t* value);

/* Replaces: graph sync inside Flame::update (row a7): vertex positions, oriented edge list,
 * edge weights, data terms.  pos 2V, edges 2E, alpha/beta E, z/wgt V, x0 V or NULL (= z),
 * tris 3T or NULL.  State is reset to x = x0, w = 0, x_bar = x, w_bar = 0, q = 0. */
int flame_hip_graph_upload(flame_hip_graph* g, const float* pos, const int32_t* edges,
                           const float* alpha, const float* beta, const float* z,
                           const float* wgt, const float* x0, const int32_t* tris);

/* Replaces: graph sync inside Flame::update (row a7) when the caller has the tracked features and
 * their Delaunay triangulation rather than a ready edge list: derives the unique undirected edges
 * (i < j, lexicographic), alpha = beta = 1/|pos_i - pos_j|, the data terms z = mu / scale with
 * scale = mean(mu) under rescale_data, the data weights (1 or 1/var) and the initial x (prediction
 * / scale where init_with_prediction and the prediction is finite, else z), resizes the handle to
 * (V, E, T) and uploads.  Parameters: reference src/flame_offline_tum.cc:234-249,
 * cfg/flame_offline_tum.yaml:87-92.  Every feature must pass the gate var < idepth_var_max_graph
 * (FLAME_HIP_ERR_ARG otherwise; flame_hip_feature_gate selects them BEFORE triangulation).
 * The solve then runs in rescaled units; flame_hip_scale_state(g, scale) brings the state back. */
typedef struct {
  int32_t adaptive_data_weights; /* regularization/nltgv2/adaptive_data_weights */
  int32_t rescale_data;          /* .../rescale_data */
  int32_t init_with_prediction;  /* .../init_with_prediction */
  float idepth_var_max_graph;    /* .../idepth_var_max */
  /* [UPSTREAM-RECALL] switches; an all-zero tail is the default.  edge_weight_rule 0: alpha = beta =
   * 1/|pos_i - pos_j|; 1: alpha = beta = 1; 2: alpha = 1/len, beta = 1; 3: alpha = 1, beta = 1/len.
   * alpha_gain / beta_gain multiply the rule's value (0 reads 1).  Any non-default value takes the
   * host sync path.  (Caller-supplied weights: flame_hip_graph_upload.) */
  int32_t edge_weight_rule;
  float alpha_gain, beta_gain;
} flame_hip_sync_params;
int flame_hip_graph_sync(flame_hip_graph* g, const flame_hip_sync_params* sp, int32_t V, int32_t T,
                         const float* pos, const float* idepth_mu, const float* idepth_var,
                         const int32_t* tris, const float* prediction, float* scale);
/* Row f3's first leg -- the Delaunay triangulation of a frame's features, on the GPU (the reference budgets it as
 * `triangulate` beside `sync_graph`, msg/FlameStats.msg:43-44; upstream calls Shewchuk's Triangle on the host; the
 * host triangulator of the same contract is include/flame/utils/delaunay.h).  pos: V x {u, v} pixel coordinates
 * (|u|, |v| < 2^13, snapped to a 2^-16 pixel lattice; exact predicates, so pixel lattices and collinear runs are
 * ordinary inputs).  tris receives *T <= tri_cap (2V always suffices) counter-clockwise triangles -- (b - a) x (c - a)
 * > 0 in these coordinates --, each starting at its smallest vertex, ordered by that vertex; cocircular points are cut
 * as a fan from their smallest id, points that coincide after snapping are triangulated once (smallest id).  The
 * list is a function of the input alone.  Independent of the graph held by g (own scratch, the handle's staging
 * stream); returns when the list is in tris.  Errors: ARG (coordinate out of range, tri_cap too small), NAN, STATE
 * (no device; or the result failed Euler's check T = 2 n - 2 - h: never seen, reported rather than handed out).
 * flame_hip_get_info: "delaunay_hull" (h), "delaunay_live" (n), "delaunay_us" (host time of the call).
 * A flame_hip_graph_sync on the same handle with the same V and T and tris = NULL uses this list as the library still
 * holds it -- on the DEVICE (r05): nothing of it crosses the host link on the frame path.
 * KEEP mode, tri_cap = 0 and tris = NULL: only *T comes back (one round trip behind the last kernel); the list stays on the
 * device for that graph sync and its host copy travels on a stream of its own meanwhile -- flame_hip_delaunay_list hands
 * it out (and waits for it) when the caller wants the triangles, e.g. while the GPU iterates. */
int flame_hip_delaunay(flame_hip_graph* g, int32_t V, const float* pos, int32_t tri_cap, int32_t* tris, int32_t* T);
int flame_hip_delaunay_list(flame_hip_graph* g, int32_t tri_cap, int32_t* tris);
/* keep[v] = var[v] < var_max; returns the number kept (or a negative error).  No device needed. */
int32_t flame_hip_feature_gate(int32_t n, const float* idepth_var, float var_max, uint8_t* keep);
/* The edge list flame_hip_graph_sync derived (2E ints; E from flame_hip_get_info "E"). */
int flame_hip_graph_edges(const flame_hip_graph* g, int32_t* edges);
/* x, w, x_bar, w_bar and z times s (asynchronous on the handle's stream). */
int flame_hip_scale_state(flame_hip_graph* g, float s);

/* New frame on an UNCHANGED topology (same vertices, edges, weights): only the data terms, data
 * weights and the initial x change.  Resets the state exactly like flame_hip_graph_upload but
 * keeps the host plan, the device graph arrays and the captured launch graphs.  z/wgt V, x0 V or
 * NULL (= z). */
int flame_hip_graph_update_data(flame_hip_graph* g, const float* z, const float* wgt, const float* x0);

/* Frames axis: a batch of `num_graphs` INDEPENDENT graphs in one handle (block-diagonal): graph b
 * owns the vertices [voff[b], voff[b+1]) (voff has num_graphs+1 entries, voff[0] = 0,
 * voff[num_graphs] = V); edge endpoints are vertex ids of the concatenated arrays and must stay
 * inside one graph.  Every graph becomes one LDS-resident tile, so one launch runs ALL iterations
 * of ALL frames (one workgroup per frame); a graph too large for one tile -> FLAME_HIP_ERR_ARG.
 * Same array conventions as flame_hip_graph_upload. */
int flame_hip_graph_upload_batch(flame_hip_graph* g, int32_t num_graphs, const int32_t* voff,
                                 const float* pos, const int32_t* edges, const float* alpha,
                                 const float* beta, const float* z, const float* wgt,
                                 const float* x0, const int32_t* tris);

/* Overwrite solver state (any pointer may be NULL = keep).  q is 3E interleaved. */
int flame_hip_set_state(flame_hip_graph* g, const float* x, const float* w1, const float* w2,
                        const float* xb, const float* w1b, const float* w2b, const float* q);

/* Replaces: the loop of nltgv2_l1_graph_regularizer::step() calls (rows a2-a5).  Asynchronous on
 * the handle's stream unless stream != NULL (a hipStream_t), in which case it runs there. */
int flame_hip_solve(flame_hip_graph* g, const flame_hip_params* p, int32_t num_iters,
                    void* stream);
int flame_hip_sync(flame_hip_graph* g);
/* Device time of the last flame_hip_solve in ms (HIP events on the solve's stream) and the
 * number of kernel launches it made.  Synchronises. */
int flame_hip_last_solve_ms(flame_hip_graph* g, float* ms, int32_t* launches);

/* Row a9: the optional graph filters applied to the vertex idepths (upstream options
 * regularization/do_median_filter, do_lowpass_filter, reference cfg/flame_offline_tum.yaml:85-86;
 * timing keys median_filter / lowpass_filter, msg/FlameStats.msg:45-46).  kind 0 = median of the
 * vertex and its neighbours (lower median), kind 1 = plain average of the vertex and its
 * neighbours; `passes` Jacobi passes; sets x and x_bar.  Asynchronous on the handle's stream. */
int flame_hip_graph_filter(flame_hip_graph* g, int32_t kind, int32_t passes);

/* Replaces: smoothnessCost()/dataCost() behind the stat keys nltgv2_total_smoothness_cost and
 * nltgv2_total_data_cost (reference src/utils.cc:131-136).  Synchronises. */
int flame_hip_costs(flame_hip_graph* g, const flame_hip_params* p, double* smooth, double* data);
/* The same sums restricted to flagged vertices (vmask, V bytes, caller's order, NULL = all) and
 * edges (emask, E bytes, NULL = all): a multi-GPU subdomain sums what it OWNS and the
 * ranks all-reduce the two doubles ("final cost reduction: one ncclAllReduce of 2 doubles"). */
int flame_hip_costs_masked(flame_hip_graph* g, const flame_hip_params* p, const uint8_t* vmask,
                           const uint8_t* emask, double* smooth, double* data);

/* Replaces: the per-triangle stage feeding getInverseDepthMesh (row a8).  Kinv row-major 3x3.
 * Outputs (any may be NULL): vtx_normals 3V, tri_valid T, tri_normals 3T.  Synchronises. */
int flame_hip_triangles(flame_hip_graph* g, const float Kinv[9], const flame_hip_tri_params* tp,
                        float* vtx_normals, uint8_t* tri_valid, float* tri_normals);

/* Everything flame::Flame::update() reads back after flame_hip_solve, in one call with ONE stream
 * synchronisation: the two costs (in the solver's units, i.e. before scale_back is applied), then
 * the state times scale_back (1 = leave it; rescale_data: the scale flame_hip_graph_sync returned),
 * the idepths x (V), the per-triangle stage (vtx_normals 3V, tri_valid T) and the edge list derived
 * by flame_hip_graph_sync (2E), and the stat key `coverage` (reference src/utils.cc:122): the share
 * of the tp->width x tp->height pixels the FILTERED dense idepthmap covers (not NaN).  Any output
 * pointer may be NULL.  Synchronises.  The un-scaling is
 * applied to the resident state in place and only ONCE per upload: on a state that is already back
 * in the caller's units (an earlier call, or flame_hip_scale_state) scale_back is ignored and asking
 * for the costs returns FLAME_HIP_ERR_STATE. */
int flame_hip_frame_results(flame_hip_graph* g, const flame_hip_params* p, float scale_back,
                            const float Kinv[9], const flame_hip_tri_params* tp, double* smooth,
                            double* data, float* x, float* vtx_normals, uint8_t* tri_valid,
                            int32_t* edges, float* coverage);

/* Debug images of flame::Flame rendered ON THE DEVICE (reference src/flame_offline_tum.cc:731-766;
 * what each shows: cfg/flame_offline_tum.yaml:58-64): BGR8, tp->width x tp->height, row-major, on
 * black.  WIREFRAME: sides of the valid triangles coloured by idepth; FEATURES: 3x3 squares at the
 * n_feat raw features (feat_pos 2 n_feat, feat_mu n_feat; ignored by the other kinds) coloured by
 * idepth; NORMALS: "image colored by interpolated normal vectors" over the filtered dense map;
 * IDEPTHMAP: jet of the filtered dense idepthmap.  Colour = jet(idepth * scene_color_scale, 0, 2)
 * (output/scene_color_scale, cfg/flame_offline_tum.yaml:35).  The exact rules are stated in
 * oracle/nltgv2_oracle.c (the block above nltgv2_coverage).  Positions need no validation by the
 * caller: a coordinate becomes a pixel by exact half-away-from-zero rounding, and only after a float
 * test of its reach -- a triangle side is drawn iff all four coordinates of its end points lie in
 * [-(W + H), 2 (W + H)], a feature iff -2 < u < W + 1 and -2 < v < H + 1 -- so NaN, infinite and huge
 * positions draw nothing.  Nothing is drawn on the host; the dense raster is
 * shared with flame_hip_frame_results' coverage and flame_hip_depthmaps.  Synchronises. */
enum { FLAME_HIP_IMG_WIREFRAME = 0, FLAME_HIP_IMG_FEATURES = 1, FLAME_HIP_IMG_NORMALS = 2, FLAME_HIP_IMG_IDEPTHMAP = 3 };
int flame_hip_debug_image(flame_hip_graph* g, int32_t kind, const float Kinv[9],
                          const flame_hip_tri_params* tp, float scene_color_scale, int32_t n_feat,
                          const float* feat_pos, const float* feat_mu, uint8_t* bgr);

/* "Next" row f1: the mesh as flame_ros publishes it on /flame/mesh.  Replaces the
 * vertex loop and face loop of publishDepthMesh (reference src/utils.cc:184-230): points = V x 12
 * floats in flame_ros::PointNormalUV layout {x,y,z,0 | nx,ny,nz,0 | u/(W-1), v/(H-1), 0, 0}
 * (reference src/utils.h:47-53), NaN xyz for vertices whose idepth is NaN or <= 0; faces = valid
 * triangles with reversed winding, 3 vertex ids each (capacity 3T), *num_faces of them.  Runs the
 * triangle stage first.  Any output pointer may be NULL.  Synchronises. */
int flame_hip_mesh(flame_hip_graph* g, const float Kinv[9], const flame_hip_tri_params* tp,
                   float* points, int32_t* faces, int32_t* num_faces);

/* "Next" row f2: dense maps at tp->width x tp->height (row-major, any output may
 * be NULL).  idepthmap replaces getInverseDepthMap() (filtered = 0, reference
 * src/flame_nodelet.cc:688) / getFilteredInverseDepthMap() (filtered = 1: only valid triangles,
 * reference src/flame_offline_tum.cc:643): barycentric idepth of the lowest-index covering
 * triangle, NaN where uncovered.  depthmap replaces the OpenMP inversion loop (reference
 * src/flame_offline_tum.cc:650-661): 1/idepth where idepth is not NaN and > 0, else NaN.  cloud
 * (3 floats per pixel) replaces publishPointCloud's loop (reference src/utils.cc:290-312): NaN if
 * depth is NaN or outside [min_depth, max_depth], else Kinv (jj d, ii d, d).  Synchronises. */
int flame_hip_depthmaps(flame_hip_graph* g, const float Kinv[9], const flame_hip_tri_params* tp,
                        int32_t filtered, float min_depth, float max_depth, float* idepthmap,
                        float* depthmap, float* cloud);

/* The prediction stage (upstream's `project_graph`, a timing key of reference src/utils.cc:143-156; the algorithm is this
 * build's own statement, DESIGN.md 5.4, restated operation by operation in tests/predict_ref.py, which the GPU equals bit for
 * bit): the mesh the handle STILL HOLDS from the previous frame -- vertex pixels, idepths in the caller's units (i.e. behind
 * flame_hip_frame_results / flame_hip_scale_state under rescale_data), triangles, tri_valid of the last triangle stage run on
 * the handle -- is warped by T_cur_prev = T_world_cur^-1 T_world_prev (row-major 3x4 [R|t] in double) into the current view of
 * the W x H camera K (row-major 3x3 pinhole) and z-buffered: valid triangles whose three vertices project in front of the
 * camera and that keep their orientation, nearest surface per pixel, ties to the smaller triangle id.  prediction[i] (n, may
 * be NULL) = the inverse depth of that surface's triangle evaluated at the exact query pixel pix[2i], pix[2i+1] (looked up at
 * the nearest integer pixel), NaN outside the image, on an empty pixel or when not finite and > 0; *n_finite (may be NULL) =
 * how many are finite.  This is the `prediction` flame_hip_graph_sync accepts.  n = 0 is legal: only the map is made.
 * float32 without fused multiply-add.  Reads the handle's state and changes none of it; runs on the handle's stream; synchronises.
 * Errors: ARG (NULL, W / H outside 1 .. 8192, n < 0, fx or fy <= 0), NAN (non-finite pose or K), STATE (no graph uploaded, a
 * batch of graphs, a graph without triangles, or no triangle stage -- flame_hip_triangles, _frame_results, _mesh, _depthmaps,
 * _debug_image -- since the last upload: tri_valid does not exist then), NODEVICE.
 * flame_hip_predict_map: the dense map of the last flame_hip_predict (W x H floats of THAT call, row-major): the idepth of the
 * nearest surface at every pixel centre, NaN where empty; it stays readable across later uploads.  STATE before the first one.
 * flame_hip_get_info: "predict_us" (host time of the last flame_hip_predict), "predict_device_us" (HIP events around its device work),
 * "predict_pixels" (W x H of the map flame_hip_predict_map hands out, 0 = none yet). */
int flame_hip_predict(flame_hip_graph* g, int32_t W, int32_t H, const float K[9], const double T_world_prev[12],
                      const double T_world_cur[12], int32_t n, const float* pix /* 2n */, float* prediction /* n, may be NULL */,
                      int32_t* n_finite /* may be NULL */);
int flame_hip_predict_map(flame_hip_graph* g, float* idepthmap /* W*H */);

/* The evaluate stage: the pipeline's self-check (restated operation by operation in tests/eval_ref.py, which
 * the GPU equals bit for bit).  It fills the stats the reference front ends read and nothing here set before:
 * `total_photo_error` / `avg_photo_error` (reference src/flame_offline_tum.cc:391-392, src/utils.cc:138-139) and the
 * confusion matrix of getDepthConfusionMatrix (reference src/utils.cc:326-368).  Both calls read the solver state and change
 * none of it, run on the handle's stream and synchronise once; their buffers belong to the handle and are kept across frames.
 *
 * flame_hip_photo_reference: the comparison frame -- image (H rows of W bytes, `pitch` apart) and world pose (row-major 3x4
 * [R|t] in double) --, kept on the device until replaced.  img == NULL promotes the image and pose of the last
 * flame_hip_photo_error call (no second upload; pitch and T_world_cam are not read; STATE when there is none of W x H).
 *
 * flame_hip_photo_error: every pixel (j, i) of the current image that has an idepth xi (finite, > 0) is warped by
 * T_cmp_cur = T_world_cmp^-1 T_world_cur into the comparison image, b = ((j - cx) / fx, (i - cy) / fy, 1),
 * w = A b + xi c with A = K R, c = K t formed in double and rounded once, p = (w0 / w2, w1 / w2) rounded to sixteenths of a
 * pixel; the comparison image is sampled bilinearly with integer weights (sum 256), D = |S - 256 I_cur(j, i)|.  float32
 * without fused multiply-add; the costs are integers, so the sums are exact whatever the order.  *total256 = the sum of D
 * (the photometric error in grey levels x 256); counts = pixels {evaluated, without idepth, behind the comparison camera,
 * outside it (a bilinear neighbour would be)}, which sum to W x H; error_map (W*H, may be NULL) = D / 256 per pixel, NaN where
 * not evaluated.  The map: idepthmap (host, W*H, NaN = none) or, with NULL, the handle's own dense map of the current state
 * (filtered != 0: the filtered one) -- the one rasterisation `coverage`, the map getters and the debug images share.  With a
 * caller's map only tp->width / height are read, Kinv may be NULL, and a handle without a graph is legal.
 *
 * flame_hip_truth_stats: the loop of reference src/utils.cc:339-365, branch by branch: depth_true > 0 = there is truth (NaN
 * is none), !isnan(idepth) = there is an estimate (an infinite idepth is one), error = |idepth - 1.0f / depth| resp. |idepth|.
 * confusion = {true_pos, true_neg, false_pos, false_neg}; idepth_error_map (W*H, may be NULL) = the error, NaN where the
 * reference leaves NaN.  *total_error: the reference sums the float32 errors in float32 in row-major order, which no parallel
 * kernel reproduces; here they are summed in DOUBLE in a fixed shape that depends on W x H alone (blocks of 1 024 pixels, one
 * fixed tree each, block sums added in ascending order), so the value is a function of the inputs only and within
 * 2 (W H - 1) 2^-53 of the exact sum, relatively.
 *
 * Errors: ARG (NULL, pitch < W, W / H outside 1 .. 8192, fx or fy <= 0), NAN (non-finite pose, K or Kinv) -- both before any
 * device work --, NODEVICE, STATE (photo_error before any reference or with a reference of another size; NULL map on a handle
 * without graph or triangles, or with a batch).
 * flame_hip_get_info: "photo_us" / "photo_device_us" (host time of the last flame_hip_photo_error / HIP events around its
 * device work), "photo_reference" (1 = a comparison frame is held), "truth_us" (host time of the last flame_hip_truth_stats). */
int flame_hip_photo_reference(flame_hip_graph* g, int32_t W, int32_t H, const uint8_t* img, int32_t pitch,
                              const double T_world_cam[12]);
int flame_hip_photo_error(flame_hip_graph* g, const float K[9], const float Kinv[9], const flame_hip_tri_params* tp,
                          int32_t filtered, const float* idepthmap /* host W*H, NULL = the handle's dense map */,
                          const uint8_t* img, int32_t pitch, const double T_world_cam[12],
                          uint64_t* total256, int64_t counts[4] /* evaluated, no_idepth, behind, outside */,
                          float* error_map /* W*H, may be NULL */);
int flame_hip_truth_stats(flame_hip_graph* g, const float Kinv[9], const flame_hip_tri_params* tp, int32_t filtered,
                          const float* idepthmap /* NULL = the handle's */, const float* depth_true /* host W*H */,
                          int64_t confusion[4] /* tp, tn, fp, fn */, double* total_error, float* idepth_error_map);

/* Results out (any pointer may be NULL).  Caller's vertex/edge order.  Synchronises. */
int flame_hip_download(flame_hip_graph* g, float* x, float* w1, float* w2, float* q);
int flame_hip_download_bar(flame_hip_graph* g, float* xb, float* w1b, float* w2b);

/* ---- multi-GPU subdomains: halo exchange of the solver state every D
 * iterations.  The handle holds one subdomain (own vertices + D halo rings); the caller registers
 * which of its vertices/edges (caller's ids) other ranks need (send) and which halo entries other
 * ranks own (recv).  pack/unpack move them between the solver state and a contiguous DEVICE buffer
 * (layout: n_v x {x,w1,w2,xb,w1b,w2b} then n_e x {q1,q2,q3}, float32: only what changes -- the
 * receiver holds the data terms and weights of its halo vertices since its upload) that the caller
 * hands to RCCL (ncclSend/ncclRecv, e.g. torch.distributed P2P ops).  stream: hipStream_t or NULL
 * (= the handle's stream). */
int flame_hip_halo_register(flame_hip_graph* g, int32_t n_send_v, const int32_t* send_v,
                            int32_t n_send_e, const int32_t* send_e, int32_t n_recv_v,
                            const int32_t* recv_v, int32_t n_recv_e, const int32_t* recv_e);
int flame_hip_halo_bytes(const flame_hip_graph* g, int64_t* send_bytes, int64_t* recv_bytes);
int flame_hip_halo_pack(flame_hip_graph* g, void* send_buf_dev, void* stream);
int flame_hip_halo_unpack(flame_hip_graph* g, const void* recv_buf_dev, void* stream);
/* State snapshot / rollback (device-to-device, on `stream` or the handle's) and the resident tiles' give-up word, for a
 * caller that owns the recovery of several handles at once -- the partition layer below: a give-up of ONE part cannot
 * be repeated by that handle alone (its peers already hold records of the unfinished solve), so flame_hip_part_solve
 * snapshots every part in front of the solves it queues, and flame_hip_part_sync, when any rank reports a give-up, rolls
 * every part back and repeats those solves by launches.  take_error: call after synchronising the solve's stream;
 * *gave_up = 1 when a launch of resident tiles of this handle timed out since the last look (the word is cleared, the
 * device's lease backs off; nothing is repeated here). */
/* r06, for a transport that moves the halo records itself (the partition mode's PEER transport below): the handle's state
 * arrays and registered lists as DEVICE pointers -- A / B / q [2]: {x, w1, w2, z} / {x_bar, w1_bar, w2_bar, wgt} / {q1, q2, q3, -}
 * float4 per vertex / vertex / edge, indexed by the handle's INTERNAL ids; the registered lists come in those ids too (the
 * library translated them at flame_hip_halo_register), so a transport never needs the permutation; `cur` = the buffer that
 * holds the state now.  The call orders `stream` behind any state-writing work
 * of the handle's own stream; the pointers stay valid until the next upload / resize.  flame_hip_halo_written: the caller's
 * kernels on that stream have written halo state into the current buffers (what flame_hip_halo_unpack does itself). */
typedef struct {
  void* A[2];
  void* B[2];
  void* q[2];
  int32_t cur;
  int32_t n_send_v, n_send_e, n_recv_v, n_recv_e;
  const int32_t* send_v;
  const int32_t* send_e;
  const int32_t* recv_v;
  const int32_t* recv_e;
} flame_hip_halo_view;
int flame_hip_halo_view_get(flame_hip_graph* g, void* stream, flame_hip_halo_view* out);
int flame_hip_halo_written(flame_hip_graph* g);
int flame_hip_state_snapshot(flame_hip_graph* g, void* stream);
int flame_hip_state_rollback(flame_hip_graph* g, void* stream);
int flame_hip_persist_take_error(flame_hip_graph* g, int32_t* gave_up);

/* ---- partition mode without Python (BASELINE.json configs 4 / 5): ONE graph cut into world x
 * parts_per_rank subdomains by recursive coordinate bisection (METIS is not in the image), every rank solves its parts
 * with ordinary handles (resident tiles), and every halo_depth iterations the parts swap their halo records through
 * RCCL on one stream: flame_hip_halo_pack -> ncclGroupStart / ncclSend + ncclRecv per neighbouring part (a part of the
 * same rank is a send / receive of the rank with itself) / ncclGroupEnd -> flame_hip_halo_unpack.  Bit-identical to
 * the single-GPU result.  The reference has no counterpart (one CPU process, reference src/flame_offline_tum.cc:
 * 403-563).  One process per GPU; librccl.so is loaded at the first call (no link-time dependency).
 *   rank 0: flame_hip_comm_get_unique_id(id); hand `id` to every rank (MPI, a file, a socket ...);
 *   every rank: flame_hip_comm_create(&c, device, rank, world, id);
 *               flame_hip_part_create(&p, c, 0, 0, parts_per_rank, halo_depth, V, E, ... the WHOLE graph ...);
 *               flame_hip_part_solve(p, &params, iters);  flame_hip_part_costs(...);  flame_hip_part_gather(...).
 * Every rank derives all subdomains from the whole graph, so no request lists travel.  comm == NULL makes a
 * host-only plan of rank plan_rank of plan_world (tests: flame_hip_part_info / _array on it, no device, no RCCL). */
typedef struct flame_hip_comm flame_hip_comm;
typedef struct flame_hip_part flame_hip_part;
#define FLAME_HIP_COMM_ID_BYTES 128
int flame_hip_rccl_available(void); /* 1: librccl.so loads and exports every entry point this file needs */
int flame_hip_comm_get_unique_id(char id[FLAME_HIP_COMM_ID_BYTES]);
int flame_hip_comm_create(flame_hip_comm** out, int device, int rank, int world, const char id[FLAME_HIP_COMM_ID_BYTES]);
void flame_hip_comm_destroy(flame_hip_comm* c); /* destroy the parts built on it FIRST (a part keeps the pointer) */
void* flame_hip_comm_stream(flame_hip_comm* c); /* the hipStream_t everything of this communicator is ordered on */
int flame_hip_part_create(flame_hip_part** out, flame_hip_comm* comm, int32_t plan_rank, int32_t plan_world,
                          int32_t parts_per_rank, int32_t halo_depth, int32_t V, int32_t E, const float* pos,
                          const int32_t* edges, const float* alpha, const float* beta, const float* z,
                          const float* wgt, const float* x0 /* or NULL */);
void flame_hip_part_destroy(flame_hip_part* p);
/* num_iters more PD iterations, an exchange whenever the halo rings are used up; asynchronous on the communicator's
 * stream (no host synchronisation inside); successive calls continue on the rings the last one left */
int flame_hip_part_solve(flame_hip_part* p, const flame_hip_params* params, int32_t num_iters);
/* Waits for everything queued.  COLLECTIVE when world > 1 (one 4-byte ncclAllReduce): the ranks agree whether any launch
 * of resident tiles gave up since the last synchronising call; if so EVERY rank rolls its parts back to the snapshot taken
 * in front of the first solve since then and repeats those solves by ordinary launches (info "recovered" counts them) --
 * a give-up costs time, never the result.  _costs, _gather and _update_data synchronise through this call. */
int flame_hip_part_sync(flame_hip_part* p);
/* "rank", "world", "rccl_ranks" (what RCCL itself reports: ncclCommCount), "device" */
int flame_hip_comm_info(const flame_hip_comm* c, const char* key, int64_t* value);
/* new frame on the unchanged topology: data terms, weights, initial x of the WHOLE graph (x0 NULL = z); state reset */
int flame_hip_part_update_data(flame_hip_part* p, const float* z, const float* wgt, const float* x0);
/* the whole graph's cost terms: owned sums of every part + one ncclAllReduce of 2 doubles.  Synchronises. */
int flame_hip_part_costs(flame_hip_part* p, const flame_hip_params* params, double* smooth, double* data);
/* the whole solution on every rank (x, w1, w2: V; q: 3E interleaved; any may be NULL).  Synchronises. */
int flame_hip_part_gather(flame_hip_part* p, float* x, float* w1, float* w2, float* q);
/* r06 PEER TRANSPORT ("transport" 1; 0 = RCCL, the default and the contract's path): the records of an exchange are written
 * by ONE kernel of the sending rank straight into the receiving parts' inboxes -- uncached device memory of the same GPU, of
 * another process (hipIpc) or of another GPU of the node (peer access over xGMI) --, a per-message flag word takes the exchange's
 * epoch behind them (release, system scope), and ONE kernel of the receiving rank waits for its flags (bounded) and unpacks:
 * two launches per exchange whatever the number of parts and neighbours, no host synchronisation, no ncclGroup (35-70 us on
 * one GPU against ~20 us of resident compute per 16 iterations: profiles/r05_part_halo_depth.txt).  Two record buffers by
 * epoch parity (a sender can be at most one exchange ahead).  Same bits.  Ranks of ONE process / world 1 need nothing else;
 * ranks in different processes exchange their inbox handles once: every rank calls flame_hip_part_peer_blob, the application
 * gathers the blobs of all ranks in rank order (the library does it itself over RCCL when the communicator has one:
 * flame_hip_part_set_option "transport" 1 is then collective) and hands them to flame_hip_part_peer_connect.
 * flame_hip_comm_create_local: a communicator WITHOUT RCCL for that case (peer transport only; flame_hip_part_costs then
 * returns this rank's owned sums, and the parts solve by launches -- the give-up agreement of resident tiles is an all-reduce). */
#define FLAME_HIP_PEER_BLOB_BYTES 128
int flame_hip_comm_create_local(flame_hip_comm** out, int device, int rank, int world);
int flame_hip_part_peer_blob(flame_hip_part* p, char blob[FLAME_HIP_PEER_BLOB_BYTES]);
int flame_hip_part_peer_connect(flame_hip_part* p, const char* blobs /* world x FLAME_HIP_PEER_BLOB_BYTES */);
/* "transport" 0 / 1 (above); "time_exchanges" 0 / 1: HIP events around the next (up to 64) exchanges -- pack, the group of sends / receives, unpack;
 * "pipeline" (-1 = automatic, the default: on from 4 parts per rank; 0 / 1 force it; acts with parts_per_rank >= 2): inside a solve call the halo records of part i leave -- an ncclGroup of
 * their own on the communicator's second stream -- while part i + 1 iterates (overlap compute with the exchange, by
 * over-decomposition); info "exchanges_pipelined" counts them.  Same bits either way. */
int flame_hip_part_set_option(flame_hip_part* p, const char* key, int32_t value);
/* keys: "transport", "peer_connected", "num_parts", "parts_per_rank", "exchanges", "p2p_ops", "rings_left", "exchanges_timed", "exchange_ns" (mean device
 * time of the timed exchanges; synchronise first), "recovered" (solves repeated by launches after
 * a give-up of resident tiles on any rank), "persist" (the parts solve with resident tiles); per local part: "part_id",
 * "n_own", "n_ext", "e_loc", "num_peers", "send_bytes", "recv_bytes", "persist_used" (the part's LAST local solve was one launch
 * of resident tiles), "persist_launches" (how many were, so far) */
int flame_hip_part_info(const flame_hip_part* p, const char* key, int32_t local_part, int64_t* value);
/* int32 arrays: "part" (V: the part of every vertex), per local part "vid", "eid", "edges", "e_owned", "peers",
 * "send_v", "send_e", "recv_v", "recv_e", "send_cnt", "recv_cnt"; returns the element count or a negative error */
int64_t flame_hip_part_array(const flame_hip_part* p, const char* key, int32_t local_part, int32_t* out, int64_t cap);

/* ---- feature front end: what upstream's Flame::update() does in FRONT of the graph ("feature detect, epipolar
 * idepth filter") -- a camera image and a pose in, the frame's features with inverse depths out.  Upstream's code for it is not
 * in the reference tree; the algorithm is this build's own statement (DESIGN.md "Feature front end", [UPSTREAM-RECALL] where it
 * follows the paper), restated operation by operation in tests/frontend_ref.py, which the GPU equals bit for bit.  In short:
 * a feature lives at an integer pixel of a POSE FRAME with an inverse-depth prior (mu, var); every frame it is searched along
 * its epipolar segment mu +- 2 sigma in the new image (<= 257 samples, <= 1 px apart unless the cap is hit; win x win SSD of
 * 1/16-px bilinear samples as integers), the sub-sample minimum becomes an inverse-depth measurement that is fused into the
 * prior, and the feature is projected into the current frame -- at most one per detection cell is emitted (smallest variance).
 * On a pose frame every cell without an emitted feature gets a new one at its largest image gradient above min_grad_mag.
 * The handle owns a ring of max_poseframes pose-frame images on the device and max_features feature slots; all float32, no
 * fused multiply-add, integer costs.  One handle is not thread-safe.  The library reads no environment variable. */
typedef struct flame_hip_frontend flame_hip_frontend; /* opaque; owns device buffers */
typedef struct {
  int32_t detection_win_size; /* flame::Params::detection_win_size (16): side of a detection cell */
  float min_grad_mag;         /* Params::min_grad_mag (5): central-difference gradient magnitude a detection needs */
  int32_t win_size;           /* Params::zparams.win_size (5): matching window, odd, <= 9 */
  float epipolar_line_var;    /* Params::zparams.epipolar_line_var (4): px^2 of a match along the epipolar line */
  int32_t max_dropouts;       /* Params::max_dropouts (5): a feature dies when it fails more often than this in a row */
  float idepth_min, idepth_max; /* search interval clamp (0.01, 10) */
  float idepth_init, var_init;  /* prior of a new feature (0.5, 0.25) */
  float max_match_error;        /* grey^2 per window pixel above which the best match is rejected (100); with the ZSSD cost
                                 * (flame_hip_frontend_set_cost) and the gain-invariant one (_set_gain_invariant) it bounds the residual's variance per pixel, not its mean square */
} flame_hip_frontend_params;
/* status of a feature in its last frame; the first four failures are in the order they are tested */
enum {
  FLAME_HIP_FE_OK = 0,          /* matched, measurement fused, dropout counter cleared */
  FLAME_HIP_FE_NO_PARALLAX = 1, /* the search segment is shorter than 2 px: state and counter untouched */
  FLAME_HIP_FE_OUTSIDE = 2,     /* no sample's window lies inside the image (or the segment leaves the camera's front) */
  FLAME_HIP_FE_BAD_MATCH = 3,   /* best cost above max_match_error (or a degenerate measurement) */
  FLAME_HIP_FE_AMBIGUOUS = 4,   /* a sample more than 2 steps from the best costs less than 1.5 x the best */
  FLAME_HIP_FE_NEW = 5,         /* detected in this (pose) frame */
  FLAME_HIP_FE_DIED = 6,        /* dropout counter exceeded max_dropouts in this frame: the slot is free again */
  FLAME_HIP_FE_REF_GRAD = 7     /* only with flame_hip_frontend_set_ref_grad: the reference patch has no structure along the epipolar
                                 * line; no search ran, a failure like AMBIGUOUS (tested after NO_PARALLAX, before the search) */
};
void flame_hip_frontend_default_params(flame_hip_frontend_params* p);
/* K row-major 3x3 pinhole (fx = K[0], fy = K[4], cx = K[2], cy = K[5]); images arrive rectified unless a camera is set
 * (flame_hip_frontend_set_camera below).  8 <= W, H <= 8192; max_poseframes <= 64.  Device memory: (max_poseframes + 1) W H
 * bytes + ~120 bytes per feature slot (+ 3 W H bytes once a debug image is asked for).  device = -1 makes a handle without a device: arguments are checked as usual and every
 * call that needs the device returns NODEVICE. */
int flame_hip_frontend_create(flame_hip_frontend** out, int device, int32_t W, int32_t H, const float K[9], int32_t max_features,
                              int32_t max_poseframes);
void flame_hip_frontend_destroy(flame_hip_frontend* fe);
/* One frame: img = H rows of W grey bytes, `pitch` bytes apart (any pitch >= W, any alignment); T_world_cam = row-major 3x4
 * [R|t] in double.  Uploads the image, tracks every live feature against it, projects them, on a pose frame detects new ones
 * (the image joins the ring under img_id, overwriting the oldest slot once the ring is full: the features of the overwritten
 * pose frame die first), compacts the emitted features in ascending slot order and returns when *n_out and the features are
 * on the host.  Errors: ARG (NULL, pitch < W, win_size even or > 9, ...), NAN (non-finite pose or parameter). */
int flame_hip_frontend_track(flame_hip_frontend* fe, const flame_hip_frontend_params* params, const uint8_t* img, int32_t pitch,
                             uint32_t img_id, const double T_world_cam[12], int32_t is_poseframe, int32_t* n_out);
/* The features the last frame emitted (cap >= n_out; any pointer may be NULL): vtx 2 per feature (pixel in the CURRENT frame),
 * inverse depth and variance in the current frame, slot, status (FLAME_HIP_FE_*). */
int flame_hip_frontend_features(flame_hip_frontend* fe, int32_t cap, float* vtx, float* idepth_mu, float* idepth_var, int32_t* slot,
                                int32_t* status);
/* flame::Flame::updatePoseFramePoses / prunePoseFrames (reference src/flame_nodelet.cc:474-475): new world poses (12 doubles
 * each) of pose frames by id, ids the ring does not hold are ignored; keep only the listed pose frames -- the features of
 * every other pose frame die. */
int flame_hip_frontend_set_poses(flame_hip_frontend* fe, int32_t n, const uint32_t* ids, const double* T);
int flame_hip_frontend_prune(flame_hip_frontend* fe, int32_t n, const uint32_t* keep_ids);
/* keys: "live", "poseframes", "emitted", "track_us" (host time of the last frame's call), "track_device_us" (HIP events around
 * its device work); features of the last frame per status: "ok", "no_parallax", "outside", "bad_match", "ambiguous", "new",
 * "died"; "detections_dropped" (no free slot), "max_features"; "camera" (1 = a camera is set), "ingest_device_us" (HIP events
 * around the raw upload and the ingest stage of the last _track_raw / _rectify; 0 after a _track), "ingest_raw_bytes" (what that
 * call uploaded); "gates" (bit 0 = letterbox, bit 1 = height band: what _set_gates last set), "held_height" / "refused_letterbox"
 * (features of the last frame the height band held / whose projection the letterbox refused); "cost_mode" (FLAME_HIP_FE_COST_*:
 * what _set_cost last set); "gain_invariant" (what _set_gain_invariant last set); "ref_grad" (1 while the gate of _set_ref_grad is on), "fail_ref_grad" (features of the last frame with
 * status REF_GRAD); "warp" (what _set_warp last set), "warp_refused" (features of the last frame the warped window refused);
 * "carry" (what _set_carry last set), "carried" / "carry_lost" (features of the evicted pose frame that the last frame handed over
 * to the new one / that died at the hand-over; both 0 for a frame that evicted nothing or ran with the switch off) */
int flame_hip_frontend_info(flame_hip_frontend* fe, const char* key, int64_t* value);
/* Debug/test hook: every slot's state (max_features entries each; any pointer may be NULL): alive, reference pixel (u, v),
 * ring slot of its pose frame, prior (mu, var) in the pose frame, dropout counter, last status (-1 = free), last best sample. */
int flame_hip_frontend_state(flame_hip_frontend* fe, uint8_t* alive, int32_t* u, int32_t* v, int32_t* poseframe, float* mu, float* var,
                             int32_t* dropouts, int32_t* status, int32_t* kstar);
/* Debug/test hook: the search every slot ran in the last frame (max_features entries each; any pointer may be NULL):
 * seg = {x0, y0, ex, ey} per slot (sample k of the search sits at (x0 + k ex, y0 + k ey)), steps = S (0 = no search ran).
 * steps is 0, and seg all zero, for a free slot, NO_PARALLAX, OUTSIDE decided before the segment exists and a slot a NEW feature
 * took in this frame.  Errors: ARG (NULL fe), NODEVICE, STATE before the first tracked frame. */
int flame_hip_frontend_searches(flame_hip_frontend* fe, float* seg, int32_t* steps);

/* ---- the feature pipeline's two debug images (reference cfg/flame_offline_tum.yaml:60-61: "feature detections", "epipolar line
 * searches (green success, red failure)"), rendered on the device from the record of the last tracked frame.  Integer pictures;
 * tests/fe_debug_ref.py restates the rules below and the GPU equals it byte for byte (DESIGN.md 5.3 "Debug images").
 *   Background (both): pixel (x, y) = (g, g, g), g = the tracked grey image (what flame_hip_frontend_image returns).
 *   MATCHES: a slot draws iff its status of the last frame is OK, OUTSIDE, BAD_MATCH, AMBIGUOUS or DIED and steps > 0 (alive is
 *     not consulted; a slot that died and was taken by a detection in the same frame is NEW and draws nothing).  Sample k = 0..S
 *     sits at px = x0 + (float)k ex, py = y0 + (float)k ey (float32, each operation rounded on its own, no fused multiply-add:
 *     the tracker's expression, the same bits); its pixel is X = floorf(px + 0.5f), Y = floorf(py + 0.5f), drawn only when
 *     0 <= X <= W - 1 and 0 <= Y <= H - 1, tested in float before the conversion (a NaN or infinite position draws nothing).
 *     Layer 1: every sample pixel of an OK slot, (B, G, R) = (0, 255, 0); layer 2: every sample pixel of a slot with any other
 *     drawing status, (0, 0, 255); layer 3: the pixel of sample k* of an OK slot, (0, 255, 255).  A pixel shows its highest
 *     layer, else the background.  (At the 256-step cap the samples are more than a pixel apart: the line is dotted.)
 *   DETECTIONS: every emitted feature (what flame_hip_frontend_features returns) gives a 3 x 3 filled square centred at
 *     (floorf(x + 0.5f), floorf(y + 0.5f)), clipped to the image: layer 2, (0, 255, 0), for status NEW; layer 1, (255, 0, 0), for
 *     every other emitted feature (the ones that occupy a cell, which therefore got no detection).  Highest layer wins.
 * The colour depends on the layer alone, so nothing depends on the order slots, samples or lanes arrive in. */
enum { FLAME_HIP_FE_IMG_DETECTIONS = 0, FLAME_HIP_FE_IMG_MATCHES = 1 };
/* BGR8, W x H, rows `pitch` (>= 3 W) bytes apart (bytes between the rows are left alone), of the frame the last _track / _track_raw
 * call tracked.  Rendered on the device on the front end's stream from that frame's record; set_poses / prune in between do not
 * change it.  Synchronises.  Info key "debug_image_device_us": HIP events around the last render.  Errors: ARG (NULL fe or bgr,
 * unknown kind, pitch < 3 W), NODEVICE (after the argument checks), STATE before the first tracked frame. */
int flame_hip_frontend_debug_image(flame_hip_frontend* fe, int32_t kind, uint8_t* bgr, int32_t pitch);

/* ---- ingest stage (opt-in): raw camera images in front of the tracker.  With a camera set, _track_raw takes the image as the
 * camera delivers it and runs three steps on the handle's stream between the upload and the tracker, each rounded to uint8
 * (restated in tests/ingest_ref.py, which the GPU equals bit for bit):
 *   1. grey: GRAY8 as is; BGR8 / RGB8 / BGRA8 / RGBA8 by (4899 R + 9617 G + 1868 B + 8192) >> 14, alpha ignored;
 *   2. downsample by the integer resize_factor f (1..8): W = raw_width / f, H = raw_height / f (integer division, trailing raw
 *      rows and columns ignored) must be the handle's size; pixel (x, y) = (sum of the f x f block at (f x, f y) + f f / 2) / (f f);
 *   3. undistort with the handle's K -- the K of the OUTPUT image: a caller that resizes passes K / f -- and D = (k1, k2, p1, p2,
 *      k3): distortPoint() / undistort<uint8_t>() of include/flame_ros/image_io.h operation for operation, float32 without
 *      fused multiply-add, bilinear, (uint8)(val + 0.5f).  All five coefficients exactly 0: the step is skipped.  The output is 0
 *      unless the source position (su, sv) has su > -1 && su < W && sv > -1 && sv < H, tested in float (a NaN or infinite
 *      position gives 0); inside that range taps outside the image read 0.
 * Without a camera every call does what it did before.  There is no CPU path. */
enum { FLAME_HIP_PIX_GRAY8 = 0, FLAME_HIP_PIX_BGR8, FLAME_HIP_PIX_RGB8, FLAME_HIP_PIX_BGRA8, FLAME_HIP_PIX_RGBA8 };
typedef struct {
  int32_t raw_width, raw_height, format, resize_factor;
  float D[5]; /* k1, k2, p1, p2, k3 (OpenCV order) */
} flame_hip_camera;
/* Sets the handle's camera and allocates the page-locked staging and the device buffers of the raw image; NULL: back to
 * rectified input.  Errors: ARG (size mismatch, resize_factor outside 1..8, unknown format), NAN (non-finite D), ALLOC.  On a
 * handle without a device the camera is recorded (so that the other calls check their arguments against it). */
int flame_hip_frontend_set_camera(flame_hip_frontend* fe, const flame_hip_camera* cam);
/* flame_hip_frontend_track with the ingest stage in front: raw = raw_height rows of raw_width pixels of the camera's format,
 * `pitch` bytes apart (any alignment).  Features, state, counts and info keys are those of _track on the rectified image.
 * Errors: those of _track; STATE without a camera; ARG when pitch < raw_width x bytes per pixel. */
int flame_hip_frontend_track_raw(flame_hip_frontend* fe, const flame_hip_frontend_params* params, const uint8_t* raw, int32_t pitch,
                                 uint32_t img_id, const double T_world_cam[12], int32_t is_poseframe, int32_t* n_out);
/* The stage alone: out = H rows of W rectified grey bytes, out_pitch (>= W) bytes apart.  Feature state and ring untouched. */
int flame_hip_frontend_rectify(flame_hip_frontend* fe, const uint8_t* raw, int32_t pitch, uint8_t* out, int32_t out_pitch);
/* The image the last _track / _track_raw call tracked (after the ingest stage), downloaded; STATE before the first frame. */
int flame_hip_frontend_image(flame_hip_frontend* fe, uint8_t* out, int32_t out_pitch);

/* ---- gates (opt-in): the reference's features/do_letterbox ("Process only middle third of image") and
 * regularization/nltgv2/{min_height, max_height} ("Minimum / maximum height of features that are added to graph"), evaluated in
 * the tracker and the detector (DESIGN.md 5.3 "Gates"; restated in tests/fe_gates_ref.py, which the GPU equals bit for bit).
 *   letterbox: y_lo = H / 3, y_hi = H - H / 3 (integer division).  A tracked feature whose projection has py < y_lo or py > y_hi - 1
 *     (compared in float) fails its projection exactly like one outside the image: not emitted, one dropout.  Detection candidates
 *     are restricted to the rows y_lo <= y < y_hi.  Searches and reference windows still read the whole image.
 *   height_gate: height = ((hr0 bx + hr1 by) + hr2) / idepth + h0 of a projected feature, b = K^-1 (px, py, 1), hr = up^T R and
 *     h0 = up . t of the frame's T_world_cam = [R|t] (formed in double, rounded once to float32).  Unless min_height <= height <=
 *     max_height (a NaN height fails) the feature is HELD: tracked and fused as usual, not emitted, no candidate of its cell -- a
 *     feature of larger variance in the band is emitted instead -- but its cell gets no detection.  A NEW feature is emitted ungated.
 *   up is not normalised by the library; (0, -1, 0) suits a right-down-forward world frame.
 * NULL, or both switches 0: no gate, every call does what it did before.  Takes effect with the next frame.  Valid on a handle
 * without a device.  Errors: NAN (non-finite min_height, max_height or up with height_gate != 0), ARG (NULL fe; with height_gate
 * != 0: min_height > max_height, up all zero).  A letterbox band narrower than 2 (win_size / 2 + 1) + 1 rows makes the next
 * _track / _track_raw return ARG (before any device work). */
typedef struct {
  int32_t letterbox, height_gate;
  float min_height, max_height;
  float up[3];
} flame_hip_frontend_gates;
int flame_hip_frontend_set_gates(flame_hip_frontend* fe, const flame_hip_frontend_gates* gates /* NULL = none */);

/* ---- matching cost (opt-in): what the tracker minimises along the epipolar segment (DESIGN.md 5.3 "Matching cost"; restated in
 * tests/fe_zm_ref.py, which the GPU equals bit for bit).  With D_i = sum of the bilinear weights x current pixels - 256 x
 * reference pixel over the n = win_size^2 window pixels (integers, |D_i| <= 65 280):
 *   FLAME_HIP_FE_COST_SSD (the default):  C = sum D_i^2;                    BAD_MATCH when C > bad,
 *   FLAME_HIP_FE_COST_ZSSD (zero-mean):   C = n sum D_i^2 - (sum D_i)^2;    BAD_MATCH when C > n bad (saturated at UINT64_MAX),
 * with bad = (uint64)(max_match_error win_size^2 65536).  C replaces the SSD cost in every decision -- validity, argmin (ties to
 * the smallest sample), BAD_MATCH, AMBIGUOUS, the sub-sample parabola -- and nothing else changes.  A grey offset between the
 * pose frame and the current image that clips nowhere adds 256 b to every D_i and leaves the ZSSD cost the same integer: the
 * whole tracker is bit-invariant to it (auto-exposure cameras).  A GAIN is not removed by ZSSD: a change of the exposure TIME is
 * one, and flame_hip_frontend_set_gain_invariant below removes it.  On very smooth imagery a small window
 * cannot tell a shift along a ramp from an offset: use win_size >= 7 with ZSSD.
 * Takes effect with the next _track / _track_raw and may change in mid-sequence (the feature state holds no cost).  Valid on a
 * handle without a device.  Errors: ARG (NULL fe, unknown mode). */
enum { FLAME_HIP_FE_COST_SSD = 0, FLAME_HIP_FE_COST_ZSSD = 1 };
int flame_hip_frontend_set_cost(flame_hip_frontend* fe, int32_t mode);

/* ---- gain-invariant matching cost (opt-in): auto-exposure changes the exposure time, and that is a gain.  ZSSD under a gain of
 * 0.8 has four times the median inverse-depth error and under 0.6 loses nearly every search.  With on = 1 the tracker
 * matches with the residual of the reference window after the best fit ref ~ g cur + b, anti-correlation refused (DESIGN.md 5.3
 * "Matching cost"; restated in tests/fe_gi_ref.py, which the GPU equals bit for bit).  Over the n = win_size^2 window pixels, with
 * I_i = sum of the bilinear weights x current pixels (0 ... 65 280) and R_i = 256 x reference pixel, in exact integers:
 *   ZI = n sum I^2 - (sum I)^2,  ZR = n sum R^2 - (sum R)^2,  ZIR = n sum I R - (sum I)(sum R)   (each below 2^45 in magnitude);
 *   C = ZR                                   when ZI == 0 or ZIR <= 0,
 *   C = max(0, floor(ZR - ZIR^2 / ZI))       otherwise: a double multiply, divide and subtract, each rounded once (IEEE).
 * C replaces the cost in every decision exactly as ZSSD's does; BAD_MATCH when C > n bad (ZSSD's threshold: the unit is the same),
 * and, tested before the threshold, when ZR == 0 (a flat reference window has nothing to correlate).  Nothing else changes.
 * A tracked frame I' = 2^m I + b that clips nowhere, against an unchanged pose frame, scales ZI by 4^m and ZIR by 2^m exactly, and
 * a power of two commutes with IEEE rounding: C keeps its bits, and so does everything the tracker puts out.  An offset on a pose
 * frame leaves ZR and ZIR the same integers.  A general gain is invariant up to the rounding of the 8-bit image (measured in
 * DESIGN.md 6).  A GAIN ON A POSE FRAME scales C and moves the detector: it is not claimed invariant.
 * While on it overrides the SSD / ZSSD choice of _set_cost; info key "cost_mode" keeps reporting what _set_cost set, info key
 * "gain_invariant" this switch.  Takes effect with the next _track / _track_raw and may change in mid-sequence (the feature state
 * holds no cost).  Valid on a handle without a device.  Errors: ARG (NULL fe, on outside {0, 1}); the setting then stays what it
 * was. */
int flame_hip_frontend_set_gain_invariant(flame_hip_frontend* fe, int32_t on);

/* ---- reference-patch gradient gate (opt-in): an edge parallel to the epipolar line slides along itself, every sample of the search
 * costs about the same and the minimum that gets fused is noise (the aperture problem).  With min_grad > 0 the tracker asks, after
 * the NO_PARALLAX test and before the search, whether the feature's win x win reference window has structure ALONG the line
 * (DESIGN.md 5.3 "Reference-patch gradient"; restated in tests/fe_rg_ref.py, which the GPU equals bit for bit):
 *   E = K o (homogeneous, formed in double on the host, rounded once to float32), o = R_ref^T (t_cur - t_ref): the epipole of the
 *     current view in the pose frame's image; (dx, dy) = (E0 - u E2, E1 - v E2) at the feature's pixel (u, v);
 *   Sxx, Sxy, Syy = the integer sums of gx^2, gx gy, gy^2 over the window, gx = I(x+1, y) - I(x-1, y), gy = I(x, y+1) - I(x, y-1);
 *   the feature passes iff  dx^2 Sxx + 2 dx dy Sxy + dy^2 Syy >= 4 win^2 min_grad^2 (dx^2 + dy^2)  (float32, each operation
 *     rounded on its own; a NaN refuses): the mean square of the patch's derivative along the line is at least min_grad^2.
 * A refused feature gets status FLAME_HIP_FE_REF_GRAD: no search, prior and k* = -1 untouched, search record zero, one dropout.  If
 * the one-pixel ring around the window leaves the image (win_size grew after the detection) the status is OUTSIDE.
 * min_grad = 0 (the default): off, every call does what it did before.  Takes effect with the next _track / _track_raw and may
 * change in mid-sequence.  Valid on a handle without a device.  Errors: NAN (non-finite), ARG (NULL fe, negative); after a refusal
 * the setting is what it was.  Info keys "ref_grad", "fail_ref_grad". */
int flame_hip_frontend_set_ref_grad(flame_hip_frontend* fe, float min_grad);

/* ---- warped window (opt-in): the tracker compares the reference window with an axis-aligned, unscaled window of the current
 * image, which is right only while the camera has neither rolled nor changed its distance against the pose frame: at 30 degrees of
 * roll nearly every feature is lost.  With on = 1 the current image is sampled where the reference window's pixels
 * land under the pose change, an affine 2 x 2 map J formed once per feature and frame from the pose record and the prior
 * (DESIGN.md 5.3 "Warped window"; restated in tests/fe_warp_ref.py, which the GPU equals bit for bit).  Float32, every operation
 * rounded on its own, no fused multiply-add; with a = A b, c, the clamped interval [xi0, xi1] and d0, d1 > 0 of the search:
 *   xi_J = min(max(mu, xi0), xi1) (t = mu > xi0 ? mu : xi0; xi_J = t < xi1 ? t : xi1);  w_r = a_r + xi_J c_r;  px = w0 / w2,
 *   py = w1 / w2;  gx_r = A[r][0] / fx,  gy_r = A[r][1] / fy  (r = 0, 1, 2: the derivatives of a by the reference pixel);
 *   J00 = (gx0 - px gx2) / w2,  J01 = (gy0 - px gy2) / w2,  J10 = (gx1 - py gx2) / w2,  J11 = (gy1 - py gy2) / w2.
 *   Jq = (int)floorf(J 256 + 0.5f) per entry, taken only when that float is finite and at most 1024 in magnitude (a stretch of 4),
 *   and det = Jq00 Jq11 - Jq01 Jq10 >= 4096 (an area scale of 1/16; no mirrored, no collapsed map).
 * A feature whose Jq fails either test is REFUSED before the search -- after the tests for OUTSIDE, NO_PARALLAX and REF_GRAD --:
 * status OUTSIDE, one dropout, prior and k* = -1 untouched, search record zero (the Matches image draws nothing), counted in info
 * key "warp_refused" (and in "outside").
 * Cost of sample k: q = (int)floorf(p_k 16 + 0.5f) per axis with the range test as before; for the window offset (i, j), i along x
 * and j along y, both in [-r, r]:
 *   ox = qx + ((Jq00 i + Jq01 j + 8) >> 4),  oy = qy + ((Jq10 i + Jq11 j + 8) >> 4)   (arithmetic shifts: they floor; sixteenths);
 *   I_ij = the 256-scaled bilinear sum of the current image at pixel (ox >> 4, oy >> 4) with the weights of ox & 15, oy & 15;
 *   the sample is valid only if every window pixel and its +1 neighbours lie inside the image;
 *   D_ij = I_ij - 256 ref(u + i, v + j) feeds SSD and ZSSD, I_ij the gain-invariant sums: their integer bounds hold unchanged.
 * The reference side, the gradient gate and everything behind the cost (argmin, BAD_MATCH, AMBIGUOUS, parabola, measurement,
 * fusion, projection, gates) are untouched.  Jq = (256, 0, 0, 256) gives the unwarped integers, and a pose change with R = I and
 * t_z = 0 gives exactly that Jq: on such a sequence the switch changes no bit.  A quarter turn Jq = (0, -256, 256, 0) permutes the
 * sampling positions: the cost on an image equals the unwarped cost on that image turned by 90 degrees about the sample.
 * NOT claimed: J is taken at the prior, not per sample (for a wide prior the window's scale is that of xi_J); the patch's plane is
 * taken as fronto-parallel in the pose frame, as the search itself assumes.
 * Takes effect with the next _track / _track_raw and may change in mid-sequence (the feature state holds nothing of it).  Valid on
 * a handle without a device.  Errors: ARG (NULL fe, on outside {0, 1}); the setting then stays what it was.  Info keys "warp",
 * "warp_refused". */
int flame_hip_frontend_set_warp(flame_hip_frontend* fe, int32_t on);

/* ---- hand-over (opt-in): a feature belongs to the pose frame it was detected in, and when a new pose frame takes a ring slot that
 * is in use every feature of the pose frame it overwrites dies before the frame is tracked.  A camera that hovers keeps those
 * features in view, and the first pose frames hold nearly all of them: the eviction of one pose frame empties the graph
 * (DESIGN.md 6).  With on = 1 a pose frame that takes a ring slot a in use (an EVICTING frame) runs in another order (DESIGN.md 5.3
 * "Hand-over"; restated in tests/fe_carry_ref.py, which the GPU equals bit for bit); every other frame is what it was:
 *   1. the image goes into the handle's extra image slot; ring slot a keeps the old pose frame's image, and its pose record is the
 *      old pose frame's against the new pose; nothing is killed;
 *   2. tracking, detection and compaction run as they are: the old pose frame's features are tracked against the new image, take
 *      part in the cell competition and are emitted when they win their cell; new detections refer to ring slot a.  The frame's
 *      output is what these stages produce;
 *   3. behind them, every live slot of ring slot a whose status is not NEW is an old feature.  It is CARRIED iff its status is OK
 *      or NO_PARALLAX, the frame emitted it (it won its cell), and with (px, py, idepth, var) its emitted record, ur =
 *      (int)floorf(px + 0.5f), vr = (int)floorf(py + 0.5f), m = win_size / 2 + 1: m <= ur < W - m and max(m, y_lo) <= vr <
 *      min(H - m, y_hi) (y_lo, y_hi: the letterbox band, 0 and H without one) -- a pixel where a detection could sit.  A carried
 *      slot gets reference pixel (ur, vr) and prior (idepth, var), the emitted bits; its pose frame slot, dropout count, status,
 *      k* and search record stay.  Every other old feature dies (its status and search record stay; its cell stays without a
 *      feature until the next pose frame);
 *   4. the image is copied into ring slot a on the handle's stream; the slot's id and pose become the new pose frame's.
 * From the next frame on a carried feature is an ordinary feature of the new pose frame.  _prune and _set_poses are unchanged.
 * NOT claimed: the anchor moves by up to half a pixel per axis and the prior is not corrected for the surface's slope over that
 * distance; no variance is added at a hand-over.
 * Takes effect with the next evicting frame and may change between any two frames (the feature state holds nothing of it).  Valid
 * on a handle without a device.  Errors: ARG (NULL fe, on outside {0, 1}); the setting then stays what it was.  Info keys "carry",
 * "carried", "carry_lost". */
int flame_hip_frontend_set_carry(flame_hip_frontend* fe, int32_t on);

/* Debug/test hook (no device needed; works on a handle created with device = -1): copies the
 * named host-side plan array ("v_o2i", "e_o2i", "grow", "ginc", "eij", "tiles", "t_vmap",
 * "t_emap", "t_eij", "t_srow", ...) and returns its element count, or a negative error. */
int64_t flame_hip_debug_plan_array(const flame_hip_graph* g, const char* name, void* buf,
                                   int64_t cap_bytes);

const char* flame_hip_strerror(int code);
/* Library/ABI version: major*10000 + minor*100 + patch. */
int flame_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif
