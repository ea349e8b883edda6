/* hyperslam_hip.h — C ABI of the MI355X-native continuous-time NLLS backend (libhyperslam_hip.so).
 *
 * This is the drop-in boundary for HyperSLAM's optimisation hot path: everything that happens
 * inside `Optimizer<OptimizerSuite::CERES>::optimize()` -> `ceres::Solve`
 * (/root/reference/internal/hyper/optimizers/ceres/optimizer.cpp:276-280) and, per residual block, inside
 * `ExteroceptiveCost<CERES>::Evaluate` (/root/reference/internal/hyper/optimizers/ceres/costs/exteroceptive.cpp:101-160)
 * -> `Evaluator<Obs, SE3>::evaluate` (the four files under /root/reference/internal/hyper/optimizers/evaluators/).
 *
 * The reference walks a pointer graph (ceres::Problem) one residual at a time; this ABI takes the same content as
 * flat tables (control points, sensors, landmarks, per-type residual records), keeps them resident in HBM and runs
 * linearise -> robustify -> landmark Schur complement -> reduced solve -> retract -> accept/reject on the GPU.
 *
 * Conventions
 *   - plain C, opaque handle, every call returns int (0 = HS_OK); hs_last_error(handle) gives the message.
 *   - host buffers are caller-owned and only read/written during the call; device memory is library-owned.
 *   - a handle is used by one thread at a time (the reference calls its optimizer from the single backend thread,
 *     /root/reference/internal/hyper/system/components/backend.cpp:143-145); no internal host threads.
 *   - all arithmetic fp64 (/root/reference/include/hyper/optimizers/ceres/manifolds/variables/wrapper.hpp:22).
 *   - quaternions are (x, y, z, w) (su2.cpp:21, settings.yaml:34-36); a control point is the reference's
 *     Stamped<SE3> block [qx qy qz qw px py pz t] (stamped.hpp:35-36, se3.cpp:20-23).
 */
#ifndef HYPERSLAM_HIP_H_
#define HYPERSLAM_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HS_OK 0
#define HS_ERR_INVALID 1   /* bad argument / inconsistent tables */
#define HS_ERR_DEVICE 2    /* HIP runtime error */
#define HS_ERR_STATE 3     /* call order (e.g. solve before tables are set) */
#define HS_ERR_NUMERIC 4   /* non-finite values / factorisation failure surfaced to the caller */
#define HS_ERR_KNOTS 5     /* hs_set_spline: the control-point stamps are not t0 + j*dt (a hole or a shifted knot); nothing was changed */

/* Factor types = the four in-tree evaluators (optimizer.cpp:189,212,234,253). */
#define HS_PIXEL 0     /* VisualPixelEvaluator   pixel.cpp:16     2 rows, CartesianMetric, Huber(0.5)      optimizer.cpp:226 */
#define HS_BEARING 1   /* VisualBearingEvaluator bearing.cpp:14   1 row,  AngularMetric,   Huber(1.6e-3)   optimizer.cpp:204 */
#define HS_PRIOR 2     /* ManifoldEvaluator      manifold.cpp:12  6 rows, ManifoldMetric,  no loss         optimizer.cpp:250 */
#define HS_INERTIAL 3  /* InertialEvaluator      inertial.cpp:13  6 rows, CartesianMetric, Scaled(1.6e-5)  optimizer.cpp:267 */

typedef struct hs_problem hs_problem;

/* Termination (ceres::TerminationType as used by TrustRegionMinimizer). */
#define HS_NO_CONVERGENCE 0 /* max_num_iterations reached (optimizer.cpp:40: 5) */
#define HS_CONVERGENCE 1
#define HS_FAILURE 2

typedef struct hs_iteration {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_successful;
  int32_t reserved;
  double cost;              /* cost after this iteration (0.5 * sum rho(|r|^2)) */
  double cost_change;
  double gradient_max_norm; /* max |gradient| in local coordinates after this iteration's step; for the LAST executed iteration: before it */
  double step_norm;
  double relative_decrease;
  double radius;            /* trust-region radius after this iteration */
} hs_iteration;

typedef struct hs_summary {
  double initial_cost;
  double final_cost;
  int32_t num_iterations;        /* LM iterations executed (linear solves), <= max_iterations */
  int32_t num_successful_steps;
  int32_t termination;           /* HS_NO_CONVERGENCE | HS_CONVERGENCE | HS_FAILURE */
  int32_t num_residual_blocks;   /* residual blocks evaluated per linearisation on this handle */
  double linearize_ms;           /* accumulated device time per stage over the solve (HIP events); the four stage fields are -1 unless hs_set_stage_timing is on */
  double schur_ms;
  double solve_ms;
  double update_ms;
  double total_ms;
} hs_summary;

/* Output pointers for hs_linearize (each nullable). Rows are residual blocks in table order.
 * Jacobians are Ceres *local* Jacobians (J_ambient * PlusJacobian — the quantity the reference's own tests compare,
 * tests/include/tests/optimizers/evaluators/evaluator.hpp:52), row-major per residual block. */
typedef struct hs_linearization {
  double* r;            /* n x n_res                                                           */
  double* J_state;      /* n x n_res x 6k   columns: k control points x [d_rot(3) d_trans(3)]   */
  double* J_landmark;   /* n x n_res x 3    (pixel / bearing)                                   */
  double* J_bias_g;     /* n x 6 x 3kb      (inertial)                                          */
  double* J_bias_a;     /* n x 6 x 3kb      (inertial)                                          */
  double* J_gravity;    /* n x 6 x 2        (inertial; SphereManifold<3> tangent basis of Ceres) */
  int32_t* first_cp;    /* n   index of the first of the k control points used                  */
  int32_t* first_bias;  /* n   (inertial)                                                       */
  double* cost;         /* n   0.5 * rho(|r|^2)                                                 */
  /* Sensor parameter blocks (static_sensor_idx .. dynamic_sensor_idx of exteroceptive.cpp:25-99). The solver keeps them constant
   * (camera.hpp:18, imu.hpp:18, optimizer.cpp:59-64: Ceres passes nullptr); the evaluators fill them whenever the pointer is
   * non-null (bearing.cpp:74, pixel.cpp:91-135,141, manifold.cpp:57, inertial.cpp:155-194), which is what the reference's own
   * tests exercise (tests/.../evaluators/evaluator.hpp:38-65). Produced by a kernel of their own: the solver's kernels do not
   * carry them. Ceres-local like the others (extrinsics: Product(EigenQuaternion, R3) manifold, sensors/sensor.cpp:26-29). */
  double* J_extrinsics;        /* n x n_res x 6   T_bs [d_rot(3) d_trans(3)]            (all four factors) */
  double* J_intrinsics;        /* n x 2 x 4       [cx cy fx fy]                          (pixel)            */
  double* J_distortion;        /* n x 2 x 4       radtan [k1 k2 p1 p2]                   (pixel)            */
  double* J_gyro_intrinsics;   /* n x 6 x 6       i_g [c00 c11 c22 c10 c20 c21]          (inertial)         */
  double* J_acc_intrinsics;    /* n x 6 x 6       i_a                                    (inertial)         */
  double* J_gyro_sensitivity;  /* n x 6 x 9       S_g, column-major                      (inertial)         */
  double* J_acc_offsets;       /* n x 6 x 9       X_a, column-major                      (inertial)         */
} hs_linearization;

/* Exchange hook for the multi-GPU path: called once per linearisation with a device buffer of
 * `count` doubles ([S | g | cost]) that must be summed in place across ranks (RCCL all-reduce, fp64), enqueued on
 * `stream` (the handle's HIP stream). Return 0 on success. NULL = single GPU. */
typedef int (*hs_allreduce_fn)(void* user, void* device_buffer, int64_t count, void* stream);

/* ---- lifetime ---------------------------------------------------------------------------------------------- */
/* Replaces: construction of Optimizer<CERES> in Backend::Backend (backend.cpp:37-46). `stream` is a hipStream_t
 * (NULL = the library creates its own). */
int hs_create(int device, void* stream, hs_problem** out);
int hs_destroy(hs_problem* p);
const char* hs_last_error(const hs_problem* p);
/* Library/ABI version and the gfx arch the device code was built for (e.g. "gfx950"). */
int hs_version(void);
const char* hs_arch(void);

/* ---- tables (host -> HBM) ------------------------------------------------------------------------------------ */
/* Replaces swapState/updateState (optimizer.cpp:110-128, 286-345) + setStateManifold (backend.cpp:52-55):
 * uniform spline of order k (k control points per segment; BasisInterpolator(k-1, true)), control point j at stamp
 * t0 + j*dt. cp = n_cp x 8. cp_constant[j] != 0 freezes control point j (optimizer.cpp:323-328); may be NULL.
 * The quaternion of every control point must have unit norm; either sign of it is accepted and kept (q and -q are the same rotation
 * everywhere, and a solve does not change the sign a control point came with). The library neither normalises nor refuses: norms a few
 * ulp off one (what a product of unit quaternions gives) change nothing, but a norm off by e leaves the pose exact (it is normalised) and
 * puts a relative error of about 6 e into the rotation columns of every Jacobian (1e-6 -> 6e-6).
 * A table whose stamps are not t0 + j*dt is refused with HS_ERR_KNOTS (its own code: the one refusal a caller may want to survive,
 * see the plugin's optimize()); every other bad argument is HS_ERR_INVALID. */
int hs_set_spline(hs_problem* p, int order, double t0, double dt, int n_cp, const double* cp, const uint8_t* cp_constant,
                  int rotation_constant, int translation_constant);
/* Replaces setSensorManifold for cameras (optimizer.cpp:143-155; constant blocks, camera.hpp:18).
 * T_bs n x 7, intrinsics n x 4 [cx cy fx fy] (settings.yaml:38-40), distortion n x 4 radtan [k1 k2 p1 p2] (:42-45). */
int hs_set_cameras(hs_problem* p, int n, const double* T_bs, const double* intrinsics, const double* distortion);
/* Distortion model per camera: what the four distortion doubles of hs_set_cameras mean wherever a pixel is projected or un-projected
 * (pixel residuals in hs_linearize, hs_cost, hs_cost_function_evaluate, hs_reduced_system, hs_solve, hs_compute_covariance; the pixels of
 * hs_process_tracks). Bearing residuals ignore it, as they ignore intrinsics. Both models act on the plane point n = (x, y) / z, z > 0.
 *   HS_DISTORTION_RADTAN       [k1 k2 p1 p2], the default (settings.yaml:42-45)
 *   HS_DISTORTION_EQUIDISTANT  [k1 k2 k3 k4] (Kalibr pinhole-equi, OpenCV fisheye), order 4:
 *       theta = atan(|n|), d(n) = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) n / |n|        
 * models: n values, n = the camera count of hs_set_cameras; NULL (or all zeros) restores the default. An unknown value or another n is
 * HS_ERR_INVALID. The models belong to the handle like the constancy flags: hs_set_cameras with the same count keeps them, a camera table of
 * another size resets them. Cameras of different models may share a handle. hs_snapshot / hs_restore, the delta interface and camera
 * estimation leave them as they are. */
#define HS_DISTORTION_RADTAN 0
#define HS_DISTORTION_EQUIDISTANT 1
int hs_set_camera_models(hs_problem* p, int n, const int32_t* models);
/* The model of every camera of hs_set_cameras (n values). */
int hs_get_camera_models(hs_problem* p, int32_t* models);
/* Camera blocks the solver may estimate (Manifold<Sensor>::setTransformationConstant, Manifold<Camera>::setIntrinsicsConstant /
 * setDistortionConstant). constant: n x 3 flags [transformation, intrinsics, distortion] per camera, n = the camera count of
 * hs_set_cameras; non-zero keeps the block constant. NULL restores the default: every block constant (camera.hpp:18). A camera table of
 * another size resets the flags. Free coordinates are the last border unknowns, behind bias_g, bias_a, gravity and the free IMU coordinates
 * of hs_set_imu_constancy (hs_reduced_system), per camera in
 * table order the free blocks [T_bs 6 | intrinsics 4 | distortion 4], Ceres-local: T_bs on HS_MANIFOLD_SE3 [d_rot(3) d_trans(3)],
 * intrinsics [cx cy fx fy] and radtan [k1 k2 p1 p2] Euclidean. Pixel residuals touch all three blocks of their camera, bearing residuals
 * T_bs only (their intrinsics / distortion columns are zero). A camera no visual residual references is left out. At most 64 free camera
 * coordinates per window (HS_ERR_INVALID from the call that prepares the tables). hs_solve estimates the free blocks once
 * hs_set_camera_estimation has enabled it on the handle; by default it refuses a handle with free camera coordinates (HS_ERR_STATE).
 * hs_compute_covariance takes them once hs_set_camera_covariance has enabled it on the handle; by default it refuses such a handle
 * (HS_ERR_STATE). hs_solve and hs_reduced_system refuse a sharded handle (world > 1) with free camera coordinates. */
int hs_set_camera_constancy(hs_problem* p, int n, const uint8_t* constant);
/* hs_solve estimates the free camera blocks of hs_set_camera_constancy on this handle (enabled != 0). Off by default: hs_solve then refuses
 * a handle with free camera coordinates exactly as before (HS_ERR_STATE). An accepted step moves the camera table like every other variable:
 * hs_get_cameras, hs_cost, hs_linearize, hs_reduced_system, hs_process_tracks and hs_sample_trajectory see the estimate, hs_snapshot /
 * hs_restore cover it, hs_set_cameras overrides it. Such a window is solved one-ended with the camera coordinates as border columns; the border
 * (bias / gravity + camera coordinates) is limited to 137 unknowns and the window to 400 control points (HS_ERR_INVALID from the call that
 * prepares the tables, naming the limit). Handles without a free camera coordinate are not affected by the switch. DESIGN.md section 13. */
int hs_set_camera_estimation(hs_problem* p, int enabled);
/* hs_compute_covariance takes the free camera blocks of hs_set_camera_constancy on this handle (enabled != 0): their coordinates are free
 * border unknowns of the covariance, in the column order of hs_reduced_system, and the landmark blocks account for the cameras moving with
 * the landmarks. Off by default: hs_compute_covariance then refuses a handle with free camera coordinates exactly as before (HS_ERR_STATE).
 * Independent of hs_set_camera_estimation, whose limits (137 border unknowns, 400 control points) do not apply: the only limit is the 64
 * free camera coordinates of hs_set_camera_constancy. Toggling it makes a computed covariance stale. Handles without a free camera
 * coordinate are not affected by the switch. DESIGN.md section 12. */
int hs_set_camera_covariance(hs_problem* p, int enabled);
/* Current camera values in the layout of hs_set_cameras (n x 7, n x 4, n x 4): a getter of a variable table like hs_get_control_points, i.e.
 * the estimate of the last hs_solve that estimated camera blocks (after hs_restore: the snapshot) until hs_set_cameras sends the table again.
 * Each pointer may be NULL. */
int hs_get_cameras(hs_problem* p, double* T_bs, double* intrinsics, double* distortion);
/* Plain sensors (extrinsics only) used by pose-prior factors (manifold.cpp:30-33). T_bs n x 7. */
int hs_set_sensors(hs_problem* p, int n, const double* T_bs);
/* Replaces addLandmark/updateLandmarks (optimizer.cpp:347-382). xyz n x 3; constant may be NULL. */
int hs_set_landmarks(hs_problem* p, int n, const double* xyz, const uint8_t* constant);
/* Replaces setSensorManifold for the IMU (optimizer.cpp:59-64) + its bias splines (imu.cpp:64-81):
 * T_bs[7], i_g[6], i_a[6] ([c00 c11 c22 c10 c20 c21], settings.yaml:87-89), S_g[9], X_a[9] (column-major, inertial.cpp:48-49);
 * bias splines: uniform R^3 splines of order bias_order, control point j at bias_t0 + j*bias_dt, n_bias x 4 [x y z t]. */
int hs_set_imu(hs_problem* p, const double* T_bs, const double* i_g, const double* i_a, const double* S_g, const double* X_a,
               int bias_order, double bias_t0, double bias_dt, int n_bias, const double* bias_g, const double* bias_a, int bias_constant);
/* IMU blocks that enter the reduced system as unknowns (Manifold<Sensor>::setTransformationConstant, Manifold<IMU>::
 * setGyroscopeIntrinsicsConstant / setAccelerometerIntrinsicsConstant, and the S_g / X_a blocks the inertial evaluator fills next to them,
 * inertial.cpp:155-194). constant: five flags [T_bs, i_g, i_a, S_g, X_a]; non-zero keeps the block constant. NULL, or
 * all five set, is the default: every block constant (imu.hpp:18), with the tables, launches and results of a handle that never calls this.
 * The flags belong to the handle: a later hs_set_imu keeps them. Free coordinates are border unknowns behind gravity and in front of the
 * free camera coordinates (hs_reduced_system), in the order of the free blocks [T_bs 6 | i_g 6 | i_a 6 | S_g 9 | X_a 9] (at most 36),
 * Ceres-local: T_bs on HS_MANIFOLD_SE3 [d_rot(3) d_trans(3)], q <- dq(delta) (x) q as for cameras; i_g / i_a [c00 c11 c22 c10 c20 c21] and
 * S_g / X_a (column-major) Euclidean in the layout of hs_set_imu. Their Jacobians follow hs_set_inertial_jacobian. A window without inertial
 * residuals leaves the IMU columns out; a coordinate whose column is zero stays, with 1 on its diagonal. hs_dim_pose and hs_reduced_system
 * (also through the delta interface) BUILD their system; hs_solve estimates the free blocks once hs_set_imu_estimation has enabled it on the
 * handle and by default refuses a handle with a free IMU block (HS_ERR_STATE) whatever hs_set_camera_estimation says. hs_compute_covariance
 * takes the free blocks once hs_set_imu_covariance has enabled it on the handle and by default refuses a handle with one (HS_ERR_STATE)
 * whatever hs_set_camera_covariance says, and hs_solve / hs_reduced_system refuse a sharded handle (world > 1) with one (HS_ERR_STATE). */
int hs_set_imu_constancy(hs_problem* p, const uint8_t* constant);
/* hs_solve estimates the free IMU blocks of hs_set_imu_constancy on this handle (enabled != 0). Off by default: hs_solve then refuses a handle
 * with a free IMU block exactly as before (HS_ERR_STATE), whatever hs_set_camera_estimation says. On: a handle whose free blocks are IMU blocks
 * only is solved; one that has free camera blocks as well needs hs_set_camera_estimation too (otherwise the camera refusal). Still refused:
 * sharded handles (world > 1), a weight matrix; hs_compute_covariance has a switch of its own (hs_set_imu_covariance). An accepted step moves the IMU parameters like every other variable:
 * hs_get_imu, hs_cost, hs_linearize, hs_reduced_system, a later hs_solve and the delta interface see the estimate, hs_snapshot / hs_restore
 * cover the five blocks, hs_set_imu overrides them (and keeps the flags). Such a window is solved one-ended with the IMU coordinates as border
 * columns; the border (bias / gravity + free IMU coordinates + the free camera coordinates of hs_set_camera_estimation) is limited to 137
 * unknowns and the window to 400 control points (HS_ERR_INVALID from the call that prepares the tables, naming the counts): a window with 17
 * bias control points (104 bias / gravity unknowns) has room for 33 of the 36 IMU coordinates. Handles without a free IMU coordinate are not
 * affected by the switch; toggling it re-prepares the tables. DESIGN.md section 14. */
int hs_set_imu_estimation(hs_problem* p, int enabled);
/* hs_compute_covariance takes the free IMU blocks of hs_set_imu_constancy on this handle (enabled != 0): their coordinates are free border
 * unknowns of the covariance, behind gravity and in front of the free camera coordinates (the column order of hs_reduced_system). Off by
 * default: hs_compute_covariance then refuses a handle with a free IMU coordinate exactly as before (HS_ERR_STATE). A switch of its own,
 * independent of hs_set_imu_estimation and of hs_set_camera_covariance: a handle that has free camera blocks as well needs
 * hs_set_camera_covariance too (otherwise the camera refusal). The limits of hs_set_imu_estimation (137 border unknowns, 400 control points)
 * do not apply. T_bs and X_a both free is refused (HS_ERR_NUMERIC): the accelerometer model a_m = a_i + diag(F_a (X_a (+) t_bs)) depends on
 * the translation of T_bs and on X_a through their sum only, so without damping their columns are exactly dependent (hs_solve, which damps,
 * estimates both). Toggling it makes a computed covariance stale. Handles without a free IMU coordinate are not affected. DESIGN.md
 * sections 12 and 14. */
int hs_set_imu_covariance(hs_problem* p, int enabled);
/* Current IMU parameters in the layout of hs_set_imu: T_bs[7], i_g[6], i_a[6], S_g[9], X_a[9]: a getter of a variable table like
 * hs_get_bias, i.e. the estimate of the last hs_solve that estimated IMU blocks (after hs_restore: the snapshot) until hs_set_imu sends the
 * parameters again. Each pointer may be NULL. HS_ERR_STATE on a handle without an IMU. */
int hs_get_imu(hs_problem* p, double* T_bs, double* i_g, double* i_a, double* S_g, double* X_a);
/* Jacobian of the inertial factor. HS_INERTIAL_AS_REFERENCE (default; also HS_REFERENCE_LITERAL=1 in the environment at hs_create)
 * reproduces inertial.cpp:131-198 as written: the linear rows of the state / extrinsic-rotation columns carry I_g where the
 * prediction has I_a (:136,142,148,158), and the S_g / X_a terms of the state, extrinsic and gravity columns are absent (:134-153,
 * 155-162,198). HS_INERTIAL_EXACT (HS_REFERENCE_LITERAL=0) is the derivative of the prediction (:200-203). The two coincide for
 * I_g = I_a, S_g = 0, X_a = 0, i.e. everywhere the reference is exercised (settings.yaml:87-96). */
#define HS_INERTIAL_AS_REFERENCE 0
#define HS_INERTIAL_EXACT 1
int hs_set_inertial_jacobian(hs_problem* p, int mode);
/* Replaces swapEnvironment gravity block + setGravityConstant (optimizer.cpp:84-108, 130-141; rule abstract.cpp:57-61). */
int hs_set_gravity(hs_problem* p, const double* g, int constant);

/* Residual tables = the content of problem_.AddResidualBlock calls (optimizer.cpp:189-274). Any order is accepted;
 * the library keeps its own landmark-major permutation and reports results in table order. */
int hs_set_pixel_residuals(hs_problem* p, int n, const double* stamps, const double* pixels, const int32_t* landmark, const int32_t* camera);
int hs_set_bearing_residuals(hs_problem* p, int n, const double* stamps, const double* bearings, const int32_t* landmark, const int32_t* camera);
int hs_set_prior_residuals(hs_problem* p, int n, const double* stamps, const double* poses, const int32_t* sensor);
int hs_set_inertial_residuals(hs_problem* p, int n, const double* stamps, const double* measurements);

/* ---- delta interface: tables kept incrementally between solves --------------------------------- */
/* The reference never rebuilds its problem: CeresOptimizer::add(...) appends one residual block when AbstractOptimizer::process hands it
 * an observation (optimizer.cpp:189-274 <- abstract.cpp:246-259, 266-292), addLandmark / updateLandmarks add and remove landmark
 * parameter blocks as the window moves (optimizer.cpp:347-382; RemoveParameterBlock takes the landmark's residual blocks along,
 * :365-371), updateState adds / removes state elements (:286-345), and optimize() only calls ceres::Solve (:276-280). The functions
 * below are that interface on the flat tables: rows are appended / retired when the caller learns of them, hs_stage() sorts and
 * uploads what changed — between solves, off optimize()'s clock — and an hs_solve() that finds the tables staged uploads nothing
 * (a control-point table re-sent with new values and the same knots costs one small copy).
 * The hs_set_* functions above remain the whole-table form of the same thing; both may be mixed.
 * The variables (control points, landmarks, bias points, gravity, and on handles that estimate them the camera table and the IMU
 * parameters) persist in the library table by table, in whatever order the calls come: a table stays at the result of the last hs_solve
 * (after hs_restore: at the snapshot) until the caller sends that table again (hs_set_spline, hs_set_landmarks, hs_set_imu for the bias
 * points and the IMU parameters, hs_set_gravity, hs_set_cameras), and re-sending one table leaves the others where they are. The getters,
 * hs_stage and every later call that evaluates the window's residuals or its spline (hs_solve, hs_cost, hs_linearize, hs_reduced_system,
 * hs_compute_covariance, hs_process_tracks, hs_sample_trajectory) see exactly that state. */
/* Rows appended to the landmark table; *first_index (nullable) receives the index of the first new row (= the landmark id the residual
 * rows refer to). Replaces addLandmark (optimizer.cpp:347-358). */
int hs_append_landmarks(hs_problem* p, int n, const double* xyz, const uint8_t* constant, int32_t* first_index);
/* Rows appended to the residual tables: same columns as hs_set_*_residuals. Replace add(...) (optimizer.cpp:189-274). */
int hs_append_pixel_residuals(hs_problem* p, int n, const double* stamps, const double* pixels, const int32_t* landmark, const int32_t* camera);
int hs_append_bearing_residuals(hs_problem* p, int n, const double* stamps, const double* bearings, const int32_t* landmark, const int32_t* camera);
int hs_append_prior_residuals(hs_problem* p, int n, const double* stamps, const double* poses, const int32_t* sensor);
int hs_append_inertial_residuals(hs_problem* p, int n, const double* stamps, const double* measurements);
/* Removes landmarks `ids` (table indices) together with every visual residual row that refers to them (updateLandmarks,
 * optimizer.cpp:360-382). The remaining landmarks keep their order and move up; remap (nullable, one entry per OLD row) receives
 * the new index of every old row, -1 for the retired ones. */
int hs_retire_landmarks(hs_problem* p, int n, const int32_t* ids, int32_t* remap);
/* Removes the rows of residual table `type` whose stamp is < stamp. (Ceres never removes prior / inertial residual blocks; the
 * plugin's retirement rule for them, include/hyper/optimizers/hip/optimizer.hpp updateLandmarks, is this call.) */
int hs_retire_residuals_before(hs_problem* p, int type, double stamp);
/* Sorts and uploads whatever changed since the tables were last staged (enqueued on the handle's stream, nothing is awaited). hs_solve
 * and the evaluation entry points stage by themselves when needed: calling this earlier only moves the work off their clock. */
int hs_stage(hs_problem* p);

/* ---- structure (bit-exact parity target) ------------------------------------------------------- */
/* Restates ExteroceptiveCost::update (exteroceptive.cpp:25-99) for residual `idx` of `type`:
 * indices[4] = {static_state_idx, static_sensor_idx, dynamic_sensor_idx, static_observation_idx},
 * sizes/offsets/block_ids have *num_blocks entries (caller provides room for 32),
 * block_ids: control-point index for state blocks, sensor id for sensor blocks, bias control-point index for bias
 * blocks, landmark id (or 0 for gravity) for the observation block. */
int hs_residual_layout(hs_problem* p, int type, int idx, int32_t* num_blocks, int32_t* indices, int32_t* sizes, int32_t* offsets,
                       int32_t* block_ids, int32_t* num_parameters, int32_t* num_residuals);

/* ---- evaluation (parity / debugging surface) ------------------------------------------------------------------ */
int hs_num_residuals(hs_problem* p, int type);
int hs_dim_pose(hs_problem* p); /* 6*n_cp (+ 6*n_bias + 2 with an IMU) (+ free IMU coordinates) (+ free camera coordinates): size of the reduced system */
/* Batched replacement of ExteroceptiveCost::Evaluate + Ceres' local-Jacobian projection for every residual of `type`.
 * robustify != 0 additionally applies Ceres' loss corrector (sqrt(rho') scaling of r and J). */
int hs_linearize(hs_problem* p, int type, int robustify, const hs_linearization* out);
/* Ceres-compatible single-block entry: same contract as
 * `bool ExteroceptiveCost::Evaluate(double const* const* parameters, double* residuals, double** jacobians)`
 * (exteroceptive.hpp:31): parameters in update() block order, jacobians[i] row-major num_residuals x size_i, nullable
 * individually or as a whole. Evaluated on the GPU at the *given* parameter values. */
int hs_cost_function_evaluate(hs_problem* p, int type, int idx, const double* const* parameters, double* residuals, double** jacobians);
/* CostConfiguration::weights (forward.hpp:30-41; exteroceptive.cpp:109-121,129-147): an n_res x n_res matrix W per factor type
 * (row-major; pixel 2, bearing 1, prior 6, inertial 6; NULL clears) with residual = W * distance(..) and J_w = W * J_m * J_e.
 * Every production call site of the reference passes weights = nullptr (optimizer.cpp:191,214,236,255), and so does the solver here:
 * the weights are honoured by the EVALUATION entry points (hs_linearize, hs_cost_function_evaluate: device rows, weighted and
 * loss-corrected per residual block on the way out); hs_solve / hs_cost / hs_reduced_system return HS_ERR_INVALID while a weight
 * matrix is set. */
int hs_set_weights(hs_problem* p, int type, const double* weights);
/* Total cost 0.5*sum rho(|r|^2) at the current point. */
int hs_cost(hs_problem* p, double* cost);
/* Reduced (landmark-eliminated), Jacobi-scaled, LM-damped system of the first iteration at the current point:
 * S (dim x dim, row-major, symmetric) and g (dim). What one LM iteration factors; parity target for the Schur build.
 * Columns: control points, then the border: bias_g points, bias_a points, gravity, free IMU coordinates (hs_set_imu_constancy), free camera
 * coordinates (hs_set_camera_constancy). */
int hs_reduced_system(hs_problem* p, double radius, double* S, double* g);

/* ---- marginal covariances (the counterpart of ceres::Covariance) ---------------------------------------- */
/* The covariance is the inverse of the undamped Gauss-Newton matrix J'J at the values the device holds (what hs_get_* return), built as the
 * solver builds it: robustified Jacobians (Ceres' loss corrector), landmarks eliminated by Schur complement, zero LM damping. Coordinates are
 * Ceres-local, the columns of hs_linearize: control points [d_rot(3) d_trans(3)], landmarks Euclidean (3), bias control points R3 each,
 * gravity the 2-dim SphereManifold basis, free IMU blocks as in hs_set_imu_constancy, free camera blocks as in hs_set_camera_constancy; the
 * border unknowns in the column order of hs_reduced_system (bias_g points, bias_a points, gravity, free IMU coordinates, free camera
 * coordinates).
 * Constant control points / landmarks / bias splines / gravity have zero covariance (as in Ceres). Camera blocks are constant unless
 * hs_set_camera_constancy frees them AND hs_set_camera_covariance is on; a handle with free camera coordinates and the switch off is refused
 * (HS_ERR_STATE). A free camera coordinate without information (the intrinsics of a camera seen through bearing rows only, say) gives
 * HS_ERR_NUMERIC naming "camera <c>, <T_bs|intrinsics|distortion> coordinate <j>". IMU blocks likewise: hs_set_imu_constancy AND
 * hs_set_imu_covariance, HS_ERR_STATE with the switch off, HS_ERR_NUMERIC naming "IMU <T_bs|i_g|i_a|S_g|X_a> coordinate <j>", and
 * HS_ERR_NUMERIC before any device work for T_bs and X_a both free (hs_set_imu_covariance).
 * A free coordinate without information (a structurally zero column, a non-positive pivot, or a pivot below 1e-12 of its Jacobi-scaled diagonal;
 * per landmark: of its scaled 3x3 block) gives HS_ERR_NUMERIC with a message naming the control point, border unknown or landmark.
 * Fixing the gauge is the caller's business: an almost singular gauge direction is not guaranteed to be caught.
 * hs_compute_covariance computes everything on the device; any later change of values or tables, hs_solve and hs_restore make it stale and the
 * getters then return HS_ERR_STATE. HS_ERR_INVALID while a weight matrix is set; HS_ERR_STATE for sharded handles (world > 1). */
int hs_compute_covariance(hs_problem* p);
/* cp_blocks n_cp x 6 x 6 (marginals); cp_band n_cp x bw x 6 x 6, entry (i, j) = block (i, i + j) (zero past the last control point,
 * bw = hs_band_blocks); landmarks n_lm x 3 x 3 (table order; NaN for a landmark without residual rows: it is not in the problem);
 * border nb x nb, nb = hs_dim_pose - 6 n_cp: bias_g points, bias_a points, gravity, then the free IMU coordinates (with
 * hs_set_imu_covariance) and the free camera coordinates (with hs_set_camera_covariance) in the column order of hs_reduced_system. Each
 * pointer is nullable. */
int hs_get_covariance(hs_problem* p, double* cp_blocks, double* cp_band, double* landmarks, double* border);
/* cp_border 6 n_cp x nb, row-major: the covariance between the control-point coordinates (rows) and the border unknowns (columns, as in
 * hs_get_covariance). Rows of constant control points and columns of constant border unknowns are zero. HS_ERR_STATE when stale. */
int hs_get_covariance_cross(hs_problem* p, double* cp_border);
/* Covariance of the pose at n stamps (n x 6 x 6, the residual coordinates of HS_PRIOR: [Log(R_m' R) ; p - p_m] with the measurement at the
 * pose itself): J(t) Sigma J(t)' over the k control points the pose depends on. HS_ERR_INVALID for a stamp outside the valid range. */
int hs_sample_covariance(hs_problem* p, int n, const double* stamps, double* cov);
/* Covariance of the SENSOR pose T_ws(t) = T_wb(t) o T_bs at n stamps (n x 6 x 6, the coordinates of hs_sample_covariance with the measurement
 * at the sensor pose). kind / index: a camera of hs_set_cameras, the IMU (index 0) or a plain sensor of hs_set_sensors (its T_bs is always
 * constant). T_bs is the value the device holds (the estimate after an hs_solve). Where the sensor's T_bs is a free unknown of the computed
 * covariance (hs_set_camera_covariance / hs_set_imu_covariance) its uncertainty and its correlation with the control points enter:
 * J_s Sigma_pp J_s' + J_s Sigma_pe J_e' + (J_s Sigma_pe J_e')' + J_e Sigma_ee J_e', J_s / J_e the state / extrinsics Jacobians of the pose
 * prior; otherwise J_s Sigma_pp J_s' alone (for an identity T_bs: hs_sample_covariance bit for bit). HS_ERR_STATE when stale, HS_ERR_INVALID
 * for a stamp outside the valid range, an unknown kind or an index outside its table. */
#define HS_SENSOR_CAMERA 0
#define HS_SENSOR_IMU 1
#define HS_SENSOR_PLAIN 2
int hs_sample_sensor_covariance(hs_problem* p, int kind, int index, int n, const double* stamps, double* cov);

/* ---- solve ------------------------------------------------------------------------------------------------------ */
/* Replaces CeresOptimizer::optimize (optimizer.cpp:276-280) with the options of optimizer.cpp:38-54 (trust-region LM,
 * Jacobi scaling, monotonic steps). iterations (nullable) receives max_iterations + 1 records (record 0 = initial point).
 * Free sensor blocks are estimated only on a handle that asked for it: free camera blocks with hs_set_camera_estimation, free IMU blocks with
 * hs_set_imu_estimation (both for a handle that has both); otherwise a handle with one is refused (HS_ERR_STATE). */
int hs_solve(hs_problem* p, int max_iterations, hs_summary* summary, hs_iteration* iterations);
/* Per-stage device times in the summary: linearize_ms / schur_ms / solve_ms / update_ms. Off by default — the four HIP events per
 * iteration that bracket the stages are barrier packets on the launch stream and cost ~5.7 us each on gfx950 (7 % of a configs[1]
 * iteration). total_ms is always measured. enabled != 0 turns the stage events on for the following hs_solve calls
 * (HS_STAGE_TIMING=1 in the environment at hs_create does the same). Visual-only solves linearise each iteration's
 * CANDIDATE (its records become the next iteration's linearisation when the step is accepted): that launch is booked under
 * linearize_ms, so that linearize_ms covers max_iterations launches of the linearisation kernel as on every other path. */
int hs_set_stage_timing(hs_problem* p, int enabled);
/* Debugging mode of the library (also HS_GUARD=1 in the environment), process wide: every device table allocated while it is on has exactly
 * the size asked for, followed by a known pattern, and hs_solve / hs_cost / hs_reduced_system / hs_linearize check the patterns of all of them
 * before they return (HS_ERR_DEVICE with the table's size if a kernel wrote past the end of one). Slow; meant for test suites. */
int hs_set_guard(int enabled);
/* Measurement switches: HS_DEBUG_FLAGS in the environment, a sum of bits read when the tables of a handle are prepared (the list, one named line per
 * switch, is csrc/switches.hpp; never needed for correct operation, most of them exist in profiling builds only). One of the product's:
 *   4294967296  (backward_sb) backward sweep of the band solve with two phases per super-step (k_band_backward_sb, the sweep up to round 6) instead of one
 *               phase on premultiplied blocks (k_band_backward_pm); same results up to rounding. */
int hs_set_allreduce(hs_problem* p, hs_allreduce_fn fn, void* user);
/* RCCL on the data path without a host hook: rank 0 obtains a 128-byte unique id (ncclGetUniqueId), the caller distributes it
 * by any means (torch.distributed in bench.py), every rank then creates its communicator (ncclCommInitRank on the handle's
 * device). From then on both per-iteration exchanges are ncclAllReduce(sum, f64, in place) enqueued on the handle's stream; the
 * hook of hs_set_allreduce, if any, is ignored. librccl.so is loaded on first use (no link-time dependency). */
int hs_rccl_unique_id(char id[128]);
int hs_rccl_init(hs_problem* p, const char id[128], int rank, int world);
/* Destroys the communicator of hs_rccl_init (no-op without one): the exchanges fall back to the hs_set_allreduce hook. Every rank
 * must call it when the collective initialisation did not succeed everywhere, so that all ranks issue the same collectives. */
int hs_rccl_shutdown(hs_problem* p);
/* What the shards exchange, read back from the library (a driver can see that RCCL really runs with N ranks): rccl_ranks = ncclCommCount
 * of the communicator of hs_rccl_init (0: none, the hs_set_allreduce hook or a single shard); doubles_per_linearisation = length of the
 * all-reduce behind every linearisation ([S | g | diag | border blocks | cost | gradient norms], valid after the first hs_solve /
 * hs_reduced_system of the current tables); doubles_per_decision = length of the second all-reduce of an iteration (5). Any pointer may
 * be NULL. */
int hs_exchange_info(hs_problem* p, int32_t* rccl_ranks, int64_t* doubles_per_linearisation, int64_t* doubles_per_decision);
/* Residual-sharded operation: this handle holds shard `rank` of `world` (all observations of a landmark on one rank,
 * control points / sensors replicated). min_band_blocks = max over ranks of hs_band_blocks() so that every rank uses the
 * same band layout for the exchanged reduced system. */
int hs_set_shard(hs_problem* p, int rank, int world, int min_band_blocks);
/* Width of the block band of the reduced system in control-point blocks (max control points touched by one landmark). */
int hs_band_blocks(hs_problem* p);
/* Device-side copy / restore of the current point, i.e. of every variable table (control points, landmarks, bias points, gravity, camera
 * values, IMU parameters): lets a caller re-run optimize() from the same window state without a host round trip (the reference's equivalent
 * is re-creating the problem). hs_restore brings back values, not settings: flags, switches and the camera models stay as they are now. It
 * needs the tables of the snapshot (HS_ERR_STATE after a change that has not been prepared, or if a table has grown since). */
int hs_snapshot(hs_problem* p);
int hs_restore(hs_problem* p);

/* ---- read back (the reference mutates the variables in place through raw double*, optimizer.cpp:299-305) ------- */
int hs_get_control_points(hs_problem* p, double* cp);
int hs_get_landmarks(hs_problem* p, double* xyz);
int hs_get_bias(hs_problem* p, double* bias_g, double* bias_a);
int hs_get_gravity(hs_problem* p, double* g);

/* ---- batched trajectory sampling (main.cpp:72-79) -------------------------------------------- */
/* Evaluates the spline at n stamps: pose n x 7 [qx qy qz qw px py pz]; velocity/acceleration (nullable) n x 6
 * [angular(3) body ; linear(3) world]. */
int hs_sample_trajectory(hs_problem* p, int n, const double* stamps, double* pose, double* velocity, double* acceleration);

/* AbstractOptimizer::process(VisualTracks) (internal/hyper/optimizers/abstract.cpp:186-264), the step right before the path:
 * pixel -> bearing conversion in both cameras of a stereo pair (Camera::convertPixelsToBearings, abstract.cpp:222-223; radtan
 * undistortion by 20 fixed-point iterations, unit norm) and triangulation of each pair into the world frame through the
 * current spline value at `stamp` (state evaluate abstract.cpp:197-198, Camera::Triangulate abstract.cpp:252: midpoint of the
 * two rays). Cameras 0 and 1 of hs_set_cameras, control points of hs_set_spline. pixels: n x 2; bearings: n x 3 (sensor
 * frames); positions_w: n x 3. Any output may be NULL. */
int hs_process_tracks(hs_problem* p, double stamp, int n, const double* pixels0, const double* pixels1, double* bearings0, double* bearings1,
                      double* positions_w);

/* ---- manifolds -------------------------------------------------------------------- */
/* The retractions the solve applies, exposed as the batched counterpart of ceres::Manifold::Plus / PlusJacobian as the reference
 * forwards them (include/hyper/optimizers/ceres/manifolds/variables/wrapper.hpp:32-38), and Minus / MinusJacobian (:44-50; never
 * called by Ceres' trust-region minimiser, provided for completeness of the Manifold interface). kind: */
#define HS_MANIFOLD_CONSTANT 0       /* SubsetManifold, all fixed (manifolds/variables/euclidean.hpp:35-36,45-50): tangent 0        */
#define HS_MANIFOLD_EUCLIDEAN 1      /* EuclideanManifold (euclidean.hpp:38), landmarks (optimizer.cpp:356): tangent = ambient     */
#define HS_MANIFOLD_CONTROL_POINT 2  /* Stamped<SE3> [q(4) p(3) t] (stamped.hpp:35-36, se3.cpp:20-23, su2.cpp:21): 8 -> 6, t fixed */
#define HS_MANIFOLD_SE3 3            /* [q(4) p(3)], sensor extrinsics (ceres/manifolds/sensors/sensor.cpp:26-29): 7 -> 6          */
#define HS_MANIFOLD_SPHERE3 4        /* SphereManifold<3>, gravity / bearings (variables/bearing.cpp:15, gravity.hpp:11-17): 3 -> 2 */
#define HS_MANIFOLD_BIAS_POINT 5     /* Stamped<R3> [b(3) t] bias control point (ceres/manifolds/sensors/imu.cpp:64-66): 4 -> 3    */
/* Tangent size of `kind` for an ambient size (only HS_MANIFOLD_CONSTANT / _EUCLIDEAN use `ambient`, 1..9), -1 if invalid. */
int hs_manifold_tangent_size(int kind, int ambient);
/* x: n x ambient, delta: n x tangent, x_plus_delta: n x ambient (Manifold::Plus, wrapper.hpp:32-34). */
int hs_manifold_plus(hs_problem* p, int kind, int ambient, int n, const double* x, const double* delta, double* x_plus_delta);
/* jacobian: n x (ambient x tangent) row-major (Manifold::PlusJacobian, wrapper.hpp:36-38). */
int hs_manifold_plus_jacobian(hs_problem* p, int kind, int ambient, int n, const double* x, double* jacobian);
/* y, x: n x ambient, y_minus_x: n x tangent (Manifold::Minus, wrapper.hpp:44-46): the tangent vector with Plus(x, .) = y. */
int hs_manifold_minus(hs_problem* p, int kind, int ambient, int n, const double* y, const double* x, double* y_minus_x);
/* jacobian: n x (tangent x ambient) row-major, d Minus(y, x) / dy at y = x (Manifold::MinusJacobian, wrapper.hpp:48-50). */
int hs_manifold_minus_jacobian(hs_problem* p, int kind, int ambient, int n, const double* x, double* jacobian);

/* ---- stereo KLT front-end (the step before hs_process_tracks) ------------------------------------------------------------------ */
/* HyperSLAM's VisualFrontend (klt.cpp: callback, trackForward, trackFeatures, selectFeatures, circularInitialization) on the device:
 * padded image pyramids, pyramidal Lucas-Kanade with a backward check, Shi-Tomasi corners with a separation mask. The arithmetic is
 * OpenCV 4's (pyrDown, calcSharrDeriv, LKTrackerInvoker, cornerMinEigenVal, goodFeaturesToTrack) with exact integer sums (DESIGN.md,
 * "Front-end: stereo KLT on the device"); parity with OpenCV itself is unpinned. A tracker has its own handle, stream and track-id
 * generator and is used by one thread at a time. Images are 8-bit, row-major, width x height of the tracker, no row padding (host memory). */
typedef struct hs_tracker hs_tracker;
typedef struct hs_tracker_options {
  int32_t max_num_tracks;        /* 150 */
  int32_t min_track_separation;  /* 30 px: disc radius of the mask and minimum corner distance */
  int32_t patch_size;            /* 21: LK window and pyramid stop size, 3..31 */
  int32_t num_pyramid_levels;    /* 3: maxLevel, i.e. levels 0..3 (fewer where a level would not exceed the patch), 0..7 */
  int32_t max_iterations;        /* 30 */
  int32_t reserved;
  double min_track_quality;      /* 0.01 */
  double max_track_error;        /* 0.5 px: forward-backward and circular checks */
  double epsilon;                /* 0.01: LK stops when |delta| <= epsilon */
  double min_eig_threshold;      /* 1e-4 */
} hs_tracker_options;
/* The defaults above (EuRoC settings.yaml of HyperSLAM, the termination criterion of klt.cpp, OpenCV's eigenvalue threshold). */
int hs_tracker_default_options(hs_tracker_options* o);
/* o may be NULL (defaults); stream NULL: the tracker creates its own. HS_ERR_INVALID for bad sizes or options, HS_ERR_DEVICE without a GPU. */
int hs_tracker_create(int device, void* stream, int width, int height, const hs_tracker_options* o, hs_tracker** out);
int hs_tracker_destroy(hs_tracker* t);
const char* hs_tracker_last_error(const hs_tracker* t);
/* buildOpticalFlowPyramid + calcSharrDeriv: levels 0..num_levels-1 unpadded, one after the other (level l is w_l x h_l bytes,
 * w_{l+1} = (w_l + 1) / 2, same for h); derivatives: int16 (dx, dy) pairs in the same order. levels / derivatives may be NULL. */
int hs_tracker_build_pyramid(hs_tracker* t, const uint8_t* image, int32_t* num_levels, uint8_t* levels, int16_t* derivatives);
/* cornerMinEigenVal (block 3, Sobel 3): width x height floats. */
int hs_tracker_min_eigen(hs_tracker* t, const uint8_t* image, float* response);
/* goodFeaturesToTrack (block 3, Shi-Tomasi): mask NULL or width x height (non-zero = allowed); corners (x, y) float pairs in acceptance
 * order, capacity max_corners (width x height if max_corners <= 0). */
int hs_tracker_good_features(hs_tracker* t, const uint8_t* image, const uint8_t* mask, int max_corners, double quality, double min_distance,
                             int32_t* n, float* corners);
/* calcOpticalFlowPyrLK image0 -> image1 with the tracker's options: points (x, y) float pairs; use_initial_flow: points1 holds the start. */
int hs_tracker_optical_flow(hs_tracker* t, const uint8_t* image0, const uint8_t* image1, int n, const float* points0, float* points1,
                            uint8_t* status, int use_initial_flow);
/* VisualFrontend::callback on one complete stereo pair (left image0, right image1). Emits the PREVIOUS frame's message: has_message = 0 on
 * the first call after create / reset; otherwise message_stamp, n tracks (capacity max_num_tracks) with ids, lengths (0 = new) and the left
 * and right pixels in that frame, float (x, y) pairs. Pairing left and right images by stamp stays with the caller. */
int hs_tracker_process(hs_tracker* t, double stamp, const uint8_t* image0, const uint8_t* image1, int32_t* has_message, double* message_stamp,
                       int32_t* n, int64_t* ids, int32_t* lengths, float* pixels0, float* pixels1);
/* Forgets the previous frame and restarts the id generator at 0. */
int hs_tracker_reset(hs_tracker* t);

#ifdef __cplusplus
}
#endif
#endif /* HYPERSLAM_HIP_H_ */
