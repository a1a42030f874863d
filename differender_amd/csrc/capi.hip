// capi.hip -- extern "C" boundary of libdifferender_hip.so (declared in include/differender_hip.h).
// Argument validation + dispatch only; kernels live in the other translation units.
#include <hip/hip_runtime.h>

#include "../../include/differender_hip.h"
#include "dr_kernels.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <unordered_map>

using namespace dr;

namespace dr {
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device, size) instead of on every launch
hipError_t allow_lds_impl(const void *kernel, size_t bytes) {
    static std::mutex mu;
    static std::unordered_map<const void *, std::unordered_map<int, size_t>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = done[kernel][dev];
    if (have >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}
}  // namespace dr

namespace {
// The library runs on the device that owns the caller's buffers, whatever the calling thread's current device is
// (autograd calls backward from another thread than forward): switch for the duration of the call, restore afterwards.
struct DeviceOf {
    int prev = -1, dev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceOf(const void *device_ptr) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, device_ptr) != hipSuccess) { (void)hipGetLastError(); return; }  // not a device pointer we know: leave as is
        dev = attr.device;
        // (a launch error somebody else left behind -- an earlier failed call of ours, another library -- must not be taken for
        // this call's: the launch functions read hipGetLastError() after their launches)
        (void)hipGetLastError();
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; return; }
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~DeviceOf() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The end of an entry whose arguments have passed their checks: switch to the device that owns device_ptr, then call the
// launch function -- a weak symbol (dr_kernels.h), null in a library linked without that kernel's object.
template <typename... Params, typename... Args>
int launch_on(const void *device_ptr, int (*launch)(Params...), Args &&...args) {
    DeviceOf guard(device_ptr);
    if (guard.err != hipSuccess) return (int)guard.err;
    if (!launch) return DR_EUNSUPPORTED;
    return launch(args...);
}

// the W buffer rows are rows [row0, row0 + W) of an image of img_W rows
bool band_fits(int W, int img_W, int row0) { return row0 >= 0 && img_W >= W && row0 <= img_W - W; }
}  // namespace

extern "C" {

// OR-ed at load time by every translation unit that was compiled with a what-if or diagnostic switch (dr_experiment.h)
int dr_experiment_flags_ = 0;

int dr_build_flags(void) { return dr_experiment_flags_; }
// a library that computes wrong results on purpose does not answer with the ABI version a loader expects
int dr_abi_version(void) { return (dr_experiment_flags_ & DR_BUILD_WRONG_RESULTS) ? -DR_ABI_VERSION : DR_ABI_VERSION; }

const char *dr_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case DR_EINVAL: return "differender_hip: invalid argument";
        case DR_EUNSUPPORTED: return "differender_hip: unsupported configuration";
        case DR_ECOLLECTIVE: return "differender_hip: RCCL reported an error";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "differender_hip: unknown error";
}

size_t dr_workspace_bytes(int n_views, int W, int H, int VX, int VY, int VZ, int R) {
    if (n_views <= 0 || W <= 0 || H <= 0 || VX < 2 || VY < 2 || VZ < 2 || R < 1) return 0;
    if (!brick_path_supported(VX, VY, VZ, R) || !brick_image_supported(W, H, VX, VY, VZ)) return 0;
    return brick_workspace_bytes(n_views, W, H, VX, VY, VZ);
}

size_t dr_workspace_bytes_tape(int n_views, int W, int H, int VX, int VY, int VZ, int R, int max_samples, float sampling_rate) {
    if (dr_workspace_bytes(n_views, W, H, VX, VY, VZ, R) == 0 || max_samples < 0 || !(sampling_rate > 0.0f)) return 0;
    return brick_workspace_bytes_tape(n_views, W, H, VX, VY, VZ, max_samples, sampling_rate);
}

int dr_ray_setup_pose_rows(const float *cam, int n_views, int W, int H, int img_W, int row0, int VX, int VY, int VZ,
                           double fov_rad, double near_plane, float sampling_rate, uint32_t jitter_seed, uint32_t view_base,
                           float *entry, float *exit_, float *rays, int32_t *nsamp, const float *pose, const float *fov_v,
                           void *stream) {
    if ((!cam && !pose) || (fov_v && !pose) || !entry || !exit_ || !rays || !nsamp) return DR_EINVAL;
    if (n_views <= 0 || W <= 0 || H <= 0 || VX < 2 || VY < 2 || VZ < 2) return DR_EINVAL;
    if (n_views > 65535 || !(sampling_rate > 0.0f)) return DR_EINVAL;
    if (!band_fits(W, img_W, row0)) return DR_EINVAL;
    DeviceOf guard(entry);
    if (guard.err != hipSuccess) return (int)guard.err;
    return (int)launch_ray_setup(cam, pose, fov_v, n_views, W, H, img_W, row0, VX, VY, VZ, fov_rad, near_plane, sampling_rate,
                                 jitter_seed, view_base, entry, exit_, rays, nsamp, (hipStream_t)stream);
}

int dr_ray_setup_rows(const float *cam, int n_views, int W, int H, int img_W, int row0, int VX, int VY, int VZ,
                      double fov_rad, double near_plane, float sampling_rate, uint32_t jitter_seed, uint32_t view_base,
                      float *entry, float *exit_, float *rays, int32_t *nsamp, void *stream) {
    if (!cam) return DR_EINVAL;
    return dr_ray_setup_pose_rows(cam, n_views, W, H, img_W, row0, VX, VY, VZ, fov_rad, near_plane, sampling_rate, jitter_seed,
                                  view_base, entry, exit_, rays, nsamp, nullptr, nullptr, stream);
}

int dr_ray_setup(const float *cam, int n_views, int W, int H, int VX, int VY, int VZ, double fov_rad,
                 double near_plane, float sampling_rate, uint32_t jitter_seed, uint32_t view_base, float *entry,
                 float *exit_, float *rays, int32_t *nsamp, void *stream) {
    return dr_ray_setup_rows(cam, n_views, W, H, W, 0, VX, VY, VZ, fov_rad, near_plane, sampling_rate, jitter_seed,
                             view_base, entry, exit_, rays, nsamp, stream);
}

// What every entry that takes ray buffers checks before any HIP call, and the MarchArgs fields they all set: the volume, the
// ray buffers and the extents. min_samples: the lowest max_samples the caller's kernels accept; finite_rate: sampling_rate
// must be finite as well as > 0. No table (R = RG = 1) and the whole image (img_W = W, row0 = 0) until the caller says
// otherwise.
static int fill_rays(MarchArgs &a, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                     int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                     const int32_t *nsamp, int n_views, int W, int H, int max_samples, int min_samples, float sampling_rate,
                     bool finite_rate) {
    if (!vol || !cam || !entry || !exit_ || !rays || !nsamp) return DR_EINVAL;
    if (vol_dtype != DR_F32 && vol_dtype != DR_F16) return DR_EINVAL;
    if (n_views <= 0 || n_views > 65535 || W <= 0 || H <= 0 || VX < 2 || VY < 2 || VZ < 2) return DR_EINVAL;
    if (max_samples < min_samples || !(sampling_rate > 0.0f) || (finite_rate && !std::isfinite(sampling_rate))) return DR_EINVAL;
    a = MarchArgs{};
    a.vol = vol; a.vol_dtype = vol_dtype; a.VX = VX; a.VY = VY; a.VZ = VZ;
    a.sx = sx; a.sy = sy; a.sz = sz; a.vol_vs = vol_view_stride;
    a.R = 1; a.RG = 1;
    a.cam = cam; a.entry = entry; a.exit_ = exit_; a.rays = rays; a.nsamp = nsamp;
    a.n_views = n_views; a.W = W; a.H = H; a.S = max_samples; a.sr = sampling_rate; a.img_W = W; a.row0 = 0;
    return 0;
}

// fill_rays and the 1-D table (the 2-D TF entries add their second axis in fill_tf2d, the depth entries their stricter
// min_samples and finite_rate in fill_depth)
static int fill_common(MarchArgs &a, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy,
                       int64_t sz, int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride,
                       const float *cam, const float *entry, const float *exit_, const float *rays,
                       const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                       int min_samples = 0, bool finite_rate = false) {
    const int rc = fill_rays(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                             W, H, max_samples, min_samples, sampling_rate, finite_rate);
    if (rc) return rc;
    if (!tf || R < 1 || tf_view_stride % 4 != 0) return DR_EINVAL;
    a.tf = tf; a.R = R; a.tf_vs = tf_view_stride;
    return 0;
}

// the fields of a backward over the forward's output out_rgba (grad_out: its upstream gradient), shared by the 1-D and the
// 2-D TF march
static int fill_bwd(MarchArgs &a, const float *grad_out, const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy,
                    int64_t dsz, int64_t dvol_view_stride, float *d_tf, int64_t dtf_view_stride) {
    if (!grad_out || !out_rgba) return DR_EINVAL;
    if (dtf_view_stride % 4 != 0) return DR_EINVAL;
    a.mode = DR_MODE_DIFF;
    a.grad_out = grad_out; a.out_fwd = out_rgba;
    a.d_vol = d_vol; a.dsx = dsx; a.dsy = dsy; a.dsz = dsz; a.dvol_vs = dvol_view_stride;
    a.d_tf = d_tf; a.dtf_vs = dtf_view_stride;
    return 0;
}

// a pose's look_from rows are the `cam` the march kernels read as the ray origin; fov_v only comes with a pose
static bool pose_fits(const float *pose, const float *fov_v) { return pose || !fov_v; }

// What the camera entries of the three marches (1-D TF, RGBA, depth; pose null: d_cam [n_views][3], else [n_views][10]) check
// once their family's fill_* has passed, before any HIP call, and the MarchArgs and CamArgs fields they all set
static int fill_camera(MarchArgs &a, CamArgs &c, double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                       const int32_t *steps, const float *grad_out, const float *out_fwd, const float *pose, const float *fov_v,
                       double *d_cam, float *d_cam_ray) {
    if (!steps || !grad_out || !out_fwd || !d_cam || !pose_fits(pose, fov_v)) return DR_EINVAL;
    if (!(near_plane > 0.0) || !(fov_rad > 0.0)) return DR_EINVAL;
    a.mode = DR_MODE_DIFF; a.pose = pose; a.fov_v = fov_v;
    a.grad_out = grad_out; a.out_fwd = out_fwd; a.fov_rad = fov_rad; a.near_plane = near_plane;
    c.jitter_seed = jitter_seed; c.view_base = view_base; c.steps = steps; c.d_cam = d_cam; c.d_cam_ray = d_cam_ray;
    return 0;
}

int dr_march_fwd_rows_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                 int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                 const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                 int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, int mode, int variant,
                 float *out_rgba, int32_t *steps, void *workspace, size_t workspace_bytes, int img_W, int row0,
                 const float *pose, const float *fov_v, void *stream) {
    MarchArgs a;
    int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam,
                         entry, exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_rgba) return DR_EINVAL;
    if (!band_fits(W, img_W, row0) || !pose_fits(pose, fov_v)) return DR_EINVAL;
    a.img_W = img_W; a.row0 = row0; a.pose = pose; a.fov_v = fov_v;
    if (mode != DR_MODE_DIFF && mode != DR_MODE_NONDIFF) return DR_EINVAL;
    const int hints = variant & ~0xff;
    variant &= 0xff;
    if (variant < DR_VARIANT_AUTO || variant > DR_VARIANT_BASELINE) return DR_EINVAL;
    if (hints & ~(DR_HINT_NO_EARLY_TERMINATION | DR_HINT_EARLY_TERMINATION | DR_COUNT_EVALUATED | DR_TAPE_TF)) return DR_EINVAL;
    if ((hints & DR_TAPE_TF) && mode != DR_MODE_DIFF) return DR_EINVAL;
    if ((hints & DR_HINT_NO_EARLY_TERMINATION) && (hints & DR_HINT_EARLY_TERMINATION)) return DR_EINVAL;
    DeviceOf guard(vol);
    if (guard.err != hipSuccess) return (int)guard.err;
    a.mode = mode; a.out = out_rgba; a.steps = steps; a.hints = hints;
    a.fov_rad = fov_rad; a.near_plane = near_plane; a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    if (variant != DR_VARIANT_BASELINE && workspace && brick_path_supported(VX, VY, VZ, R) &&
        brick_image_supported(W, H, VX, VY, VZ)) {
        if (workspace_bytes < ((hints & DR_TAPE_TF) ? brick_workspace_bytes_tape(n_views, W, H, VX, VY, VZ, max_samples, sampling_rate)
                                                    : brick_workspace_bytes(n_views, W, H, VX, VY, VZ))) return DR_EINVAL;
        if (flat_strides_ok(sx, sy, sz)) return launch_march_fwd_flat(a, (hipStream_t)stream);
    }
    // served by the plain kernels: whatever coarse tape the workspace still holds is not this call's
    if (workspace) {
        const hipError_t e = flat_invalidate_workspace(workspace, workspace_bytes, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return launch_march_fwd_baseline(a, (hipStream_t)stream);
}

int dr_march_fwd_rows(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                 int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                 const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                 int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, int mode, int variant,
                 float *out_rgba, int32_t *steps, void *workspace, size_t workspace_bytes, int img_W, int row0,
                      void *stream) {
    return dr_march_fwd_rows_pose(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                                  exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, mode,
                                  variant, out_rgba, steps, workspace, workspace_bytes, img_W, row0, nullptr, nullptr, stream);
}

int dr_march_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                 int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                 const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                 int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, int mode, int variant,
                 float *out_rgba, int32_t *steps, void *workspace, size_t workspace_bytes, void *stream) {
    return dr_march_fwd_rows(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                             exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, mode,
                             variant, out_rgba, steps, workspace, workspace_bytes, W, 0, stream);
}

int dr_march_bwd_variant(int n_views, int W, int H, int VX, int VY, int VZ, int R, int64_t sx, int64_t sy, int64_t sz,
                         int64_t dsx, int64_t dsy, int64_t dsz, int has_dvol, int variant, int has_workspace) {
    const bool fast = variant != DR_VARIANT_BASELINE && has_workspace && n_views > 0 && W > 0 && H > 0 && VX >= 2 &&
                      VY >= 2 && VZ >= 2 && R >= 1 && brick_path_supported(VX, VY, VZ, R) &&
                      brick_image_supported(W, H, VX, VY, VZ) && flat_strides_ok(sx, sy, sz) &&
                      (!has_dvol || flat_strides_ok(dsx, dsy, dsz));
    return fast ? DR_VARIANT_AUTO : DR_VARIANT_BASELINE;
}

int dr_march_bwd_rows_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                 int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                 const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                 int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, int variant,
                 const float *grad_out, const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz,
                 int64_t dvol_view_stride, float *d_tf, int64_t dtf_view_stride, void *workspace,
                 size_t workspace_bytes, int img_W, int row0, const float *pose, const float *fov_v, void *stream) {
    MarchArgs a;
    int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam,
                         entry, exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    rc = fill_bwd(a, grad_out, out_rgba, d_vol, dsx, dsy, dsz, dvol_view_stride, d_tf, dtf_view_stride);
    if (rc) return rc;
    if (!band_fits(W, img_W, row0) || !pose_fits(pose, fov_v)) return DR_EINVAL;
    a.img_W = img_W; a.row0 = row0; a.pose = pose; a.fov_v = fov_v;
    const int bwd_flags = variant & ~0xff;
    variant &= 0xff;
    if (bwd_flags & ~(DR_COUNT_EVALUATED | DR_TAPE_TF)) return DR_EINVAL;
    if ((bwd_flags & DR_TAPE_TF) && d_vol) return DR_EINVAL;   // the tape serves the TF-only backward
    if (variant < DR_VARIANT_AUTO || variant > DR_VARIANT_BASELINE) return DR_EINVAL;
    if (!d_vol && !d_tf) return 0;  // nothing requested
    DeviceOf guard(vol);
    if (guard.err != hipSuccess) return (int)guard.err;
    a.hints = bwd_flags;
    a.fov_rad = fov_rad; a.near_plane = near_plane; a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    if (dr_march_bwd_variant(n_views, W, H, VX, VY, VZ, R, sx, sy, sz, dsx, dsy, dsz, d_vol != nullptr, variant,
                             workspace != nullptr) == DR_VARIANT_AUTO) {
        if (workspace_bytes < ((bwd_flags & DR_TAPE_TF) ? brick_workspace_bytes_tape(n_views, W, H, VX, VY, VZ, max_samples, sampling_rate)
                                                        : brick_workspace_bytes(n_views, W, H, VX, VY, VZ))) return DR_EINVAL;
        return launch_march_bwd_flat(a, (hipStream_t)stream);
    }
    return launch_march_bwd_baseline(a, RayFilter{}, (hipStream_t)stream);
}

int dr_march_bwd_rows(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                 int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                 const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                 int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, int variant,
                 const float *grad_out, const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz,
                 int64_t dvol_view_stride, float *d_tf, int64_t dtf_view_stride, void *workspace,
                 size_t workspace_bytes, int img_W, int row0, void *stream) {
    return dr_march_bwd_rows_pose(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                                  exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, variant,
                                  grad_out, out_rgba, d_vol, dsx, dsy, dsz, dvol_view_stride, d_tf, dtf_view_stride, workspace,
                                  workspace_bytes, img_W, row0, nullptr, nullptr, stream);
}

int dr_march_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                 int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                 const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                 int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, int variant,
                 const float *grad_out, const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz,
                 int64_t dvol_view_stride, float *d_tf, int64_t dtf_view_stride, void *workspace,
                 size_t workspace_bytes, void *stream) {
    return dr_march_bwd_rows(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                             exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, variant,
                             grad_out, out_rgba, d_vol, dsx, dsy, dsz, dvol_view_stride, d_tf, dtf_view_stride,
                             workspace, workspace_bytes, W, 0, stream);
}

// dr_march_bwd_cam (pose null: d_cam [n_views][3]) and dr_march_bwd_pose (d_cam [n_views][10]): one implementation
static int march_bwd_camera(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                            int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                            const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                            int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, uint32_t jitter_seed,
                            uint32_t view_base, int img_W, int row0, const int32_t *steps, const float *grad_out,
                            const float *out_rgba, const float *pose, const float *fov_v, double *d_cam, float *d_cam_ray,
                            void *stream) {
    MarchArgs a;
    CamArgs c;
    int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam,
                         entry, exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    rc = fill_camera(a, c, fov_rad, near_plane, jitter_seed, view_base, steps, grad_out, out_rgba, pose, fov_v, d_cam, d_cam_ray);
    if (rc) return rc;
    if (!band_fits(W, img_W, row0)) return DR_EINVAL;
    a.img_W = img_W; a.row0 = row0;
    return launch_on(vol, launch_camera_grad, a, c, (hipStream_t)stream);
}

int dr_march_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                     int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                     const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                     int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, uint32_t jitter_seed,
                     uint32_t view_base, int img_W, int row0, const int32_t *steps, const float *grad_out,
                     const float *out_rgba, double *d_cam, float *d_cam_ray, void *stream) {
    return march_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_,
                            rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, jitter_seed, view_base,
                            img_W, row0, steps, grad_out, out_rgba, nullptr, nullptr, d_cam, d_cam_ray, stream);
}

int dr_march_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                      int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                      const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                      int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, uint32_t jitter_seed,
                      uint32_t view_base, int img_W, int row0, const int32_t *steps, const float *grad_out,
                      const float *out_rgba, const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray,
                      void *stream) {
    if (!pose) return DR_EINVAL;
    return march_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_,
                            rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, jitter_seed, view_base,
                            img_W, row0, steps, grad_out, out_rgba, pose, fov_v, d_pose, d_pose_ray, stream);
}

int dr_mse_loss_grad(const float *out_rgba, const float *reference, int64_t n, float inv_norm, float *grad_out,
                     double *loss, void *stream) {
    if (!out_rgba || !reference || n <= 0 || (!grad_out && !loss)) return DR_EINVAL;
    DeviceOf guard(out_rgba);
    if (guard.err != hipSuccess) return (int)guard.err;
    return (int)launch_mse_loss_grad(out_rgba, reference, n, inv_norm, grad_out, loss, (hipStream_t)stream);
}

// what the four image-loss entries check and copy alike
static int fill_image(ImageArgs &a, const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                      double data_range, int win_size, double win_sigma, double K1, double K2, double *stats) {
    if (!x || !y || !strides4 || !stats) return DR_EINVAL;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return DR_EINVAL;
    if (win_size < 1 || win_size > 31 || win_size % 2 == 0) return DR_EINVAL;
    if (!std::isfinite(data_range) || !(data_range > 0.0) || !std::isfinite(win_sigma) || !(win_sigma > 0.0)) return DR_EINVAL;
    if (!std::isfinite(K1) || !std::isfinite(K2)) return DR_EINVAL;
    a.x = x; a.y = y; a.N = N; a.C = C; a.H = H; a.W = W;
    for (int i = 0; i < 4; ++i) a.strides[i] = strides4[i];
    a.data_range = data_range; a.win_sigma = win_sigma; a.K1 = K1; a.K2 = K2; a.win_size = win_size;
    a.stats = stats; a.upstream = nullptr; a.grad_x = a.grad_y = nullptr;
    return 0;
}

static int fill_loss(LossArgs &a, const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                     double data_range, int win_size, double win_sigma, double K1, double K2, int flags, double *stats) {
    if (flags & ~DR_SSIM_NONNEGATIVE) return DR_EINVAL;
    a.flags = flags;
    return fill_image(a, x, y, N, C, H, W, strides4, data_range, win_size, win_sigma, K1, K2, stats);
}

int dr_dssim_mse_fwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4, double data_range,
                     int win_size, double win_sigma, double K1, double K2, int flags, double *stats, void *stream) {
    LossArgs a;
    int rc = fill_loss(a, x, y, N, C, H, W, strides4, data_range, win_size, win_sigma, K1, K2, flags, stats);
    if (rc) return rc;
    return launch_on(x, launch_dssim_mse_fwd, a, (hipStream_t)stream);
}

int dr_dssim_mse_bwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4, double data_range,
                     int win_size, double win_sigma, double K1, double K2, int flags, const double *stats,
                     const float *upstream3, float *grad_x, float *grad_y, void *stream) {
    LossArgs a;
    int rc = fill_loss(a, x, y, N, C, H, W, strides4, data_range, win_size, win_sigma, K1, K2, flags,
                       const_cast<double *>(stats));
    if (rc) return rc;
    if (!grad_x) return DR_EINVAL;
    a.upstream = upstream3; a.grad_x = grad_x; a.grad_y = grad_y;
    return launch_on(x, launch_dssim_mse_bwd, a, (hipStream_t)stream);
}

static_assert(MS_MAX_LEVELS == DR_MSSSIM_MAX_LEVELS, "dr_kernels.h and the public header disagree on the MS-SSIM levels");

static bool msssim_shape_ok(int N, int C, int H, int W, int levels) {
    return N > 0 && C > 0 && H > 0 && W > 0 && levels >= 1 && levels <= DR_MSSSIM_MAX_LEVELS;
}

size_t dr_msssim_workspace_bytes(int N, int C, int H, int W, int levels, int want_grad_y) {
    if (!msssim_shape_ok(N, C, H, W, levels)) return 0;
    return msssim_layout(N, C, H, W, levels, want_grad_y != 0).bytes;
}

static int fill_msssim(MSArgs &a, const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                       double data_range, int win_size, double win_sigma, double K1, double K2, const double *weights,
                       int levels, void *workspace, double *stats) {
    const int rc = fill_image(a, x, y, N, C, H, W, strides4, data_range, win_size, win_sigma, K1, K2, stats);
    if (rc) return rc;
    if (!weights || !msssim_shape_ok(N, C, H, W, levels)) return DR_EINVAL;
    if (std::min(H, W) <= (win_size - 1) * 16) return DR_EINVAL;   // the window fits every level of a 5-level pyramid
    for (int l = 0; l < levels; ++l)
        if (!std::isfinite(weights[l]) || !(weights[l] > 0.0)) return DR_EINVAL;
    if (!workspace && levels > 1) return DR_EINVAL;
    a.levels = levels;
    for (int l = 0; l < levels; ++l) a.weights[l] = weights[l];
    a.workspace = workspace;
    return 0;
}

int dr_msssim_mse_fwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4, double data_range,
                      int win_size, double win_sigma, double K1, double K2, const double *weights, int levels,
                      void *workspace, double *stats, void *stream) {
    MSArgs a;
    int rc = fill_msssim(a, x, y, N, C, H, W, strides4, data_range, win_size, win_sigma, K1, K2, weights, levels, workspace,
                         stats);
    if (rc) return rc;
    return launch_on(x, launch_msssim_mse_fwd, a, (hipStream_t)stream);
}

int dr_msssim_mse_bwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4, double data_range,
                      int win_size, double win_sigma, double K1, double K2, const double *weights, int levels,
                      const double *stats, const float *upstream3, float *grad_x, float *grad_y, void *workspace,
                      void *stream) {
    MSArgs a;
    int rc = fill_msssim(a, x, y, N, C, H, W, strides4, data_range, win_size, win_sigma, K1, K2, weights, levels, workspace,
                         const_cast<double *>(stats));
    if (rc) return rc;
    if (!grad_x) return DR_EINVAL;
    a.upstream = upstream3; a.grad_x = grad_x; a.grad_y = grad_y;
    return launch_on(x, launch_msssim_mse_bwd, a, (hipStream_t)stream);
}

static int fill_tv(TVArgs &a, const void *vol, int vol_dtype, int B, int D, int H, int W, const int64_t *strides4, int norm,
                   double eps) {
    if (!vol || !strides4) return DR_EINVAL;
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return DR_EINVAL;
    if (vol_dtype != DR_F32 && vol_dtype != DR_F16) return DR_EINVAL;
    if (norm != DR_TV_L1 && norm != DR_TV_ISO && norm != DR_TV_SQ) return DR_EINVAL;
    // the kernels add (float)(eps * eps): where that is 0, a flat voxel's ISO flux is 0 * inf
    if (!std::isfinite(eps) || (norm == DR_TV_ISO && !(eps > 0.0 && (float)(eps * eps) > 0.0f))) return DR_EINVAL;
    a = TVArgs{};
    a.vol = vol; a.vol_dtype = vol_dtype; a.B = B; a.D = D; a.H = H; a.W = W;
    for (int i = 0; i < 4; ++i) a.strides[i] = strides4[i];
    a.norm = norm; a.eps = eps; a.scale = 1.0f;
    return 0;
}

int dr_tv3d_fwd(const void *vol, int vol_dtype, int B, int D, int H, int W, const int64_t *strides4, int norm, double eps,
                double *sum, void *stream) {
    TVArgs a;
    int rc = fill_tv(a, vol, vol_dtype, B, D, H, W, strides4, norm, eps);
    if (rc) return rc;
    if (!sum) return DR_EINVAL;
    a.sum = sum;
    return launch_on(vol, launch_tv3d_fwd, a, (hipStream_t)stream);
}

int dr_tv3d_bwd(const void *vol, int vol_dtype, int B, int D, int H, int W, const int64_t *strides4, int norm, double eps,
                const float *upstream, float scale, float *grad, const int64_t *grad_strides4, int accumulate, void *stream) {
    TVArgs a;
    int rc = fill_tv(a, vol, vol_dtype, B, D, H, W, strides4, norm, eps);
    if (rc) return rc;
    if (!grad || !grad_strides4 || !std::isfinite(scale)) return DR_EINVAL;
    a.upstream = upstream; a.scale = scale; a.grad = grad; a.accumulate = accumulate != 0;
    for (int i = 0; i < 4; ++i) a.grad_strides[i] = grad_strides4[i];
    return launch_on(vol, launch_tv3d_bwd, a, (hipStream_t)stream);
}

// fill_common with R = RV, and what only the 2-D TF checks: the texel index RV * RG stays below 2^31, g_scale
static int fill_tf2d(MarchArgs &a, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                     int64_t vol_view_stride, const float *tf2d, int RV, int RG, int64_t tf_view_stride, float g_scale,
                     const float *cam, const float *entry, const float *exit_, const float *rays, const int32_t *nsamp,
                     int n_views, int W, int H, int max_samples, float sampling_rate) {
    const int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf2d, RV, tf_view_stride, cam, entry,
                               exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (RG < 1 || (int64_t)RV * RG >= ((int64_t)1 << 31)) return DR_EINVAL;
    if (!std::isfinite(g_scale) || !(g_scale > 0.0f)) return DR_EINVAL;
    a.RG = RG; a.g_scale = g_scale;
    return 0;
}

int dr_march_tf2d_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                      int64_t vol_view_stride, const float *tf2d, int RV, int RG, int64_t tf_view_stride, float g_scale,
                      const float *cam, const float *entry, const float *exit_, const float *rays, const int32_t *nsamp,
                      int n_views, int W, int H, int max_samples, float sampling_rate, int mode, float *out_rgba,
                      int32_t *steps, void *stream) {
    MarchArgs a;
    int rc = fill_tf2d(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf2d, RV, RG, tf_view_stride, g_scale, cam,
                       entry, exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_rgba) return DR_EINVAL;
    if (mode != DR_MODE_DIFF && mode != DR_MODE_NONDIFF) return DR_EINVAL;
    a.mode = mode; a.out = out_rgba; a.steps = steps;
    return launch_on(vol, launch_march_tf2d_fwd, a, (hipStream_t)stream);
}

int dr_march_tf2d_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                      int64_t vol_view_stride, const float *tf2d, int RV, int RG, int64_t tf_view_stride, float g_scale,
                      const float *cam, const float *entry, const float *exit_, const float *rays, const int32_t *nsamp,
                      int n_views, int W, int H, int max_samples, float sampling_rate, const float *grad_out,
                      const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                      float *d_tf2d, int64_t dtf_view_stride, void *stream) {
    MarchArgs a;
    int rc = fill_tf2d(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf2d, RV, RG, tf_view_stride, g_scale, cam,
                       entry, exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    rc = fill_bwd(a, grad_out, out_rgba, d_vol, dsx, dsy, dsz, dvol_view_stride, d_tf2d, dtf_view_stride);
    if (rc) return rc;
    if (!d_vol && !d_tf2d) return 0;  // nothing requested
    return launch_on(vol, launch_march_tf2d_bwd, a, (hipStream_t)stream);
}

int dr_march_lit_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                     int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                     const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W, int H,
                     int max_samples, float sampling_rate, const float *light, int mode, float *out_rgba, int32_t *steps,
                     void *stream) {
    MarchArgs a;
    int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_,
                         rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!light || !out_rgba) return DR_EINVAL;
    if (mode != DR_MODE_DIFF && mode != DR_MODE_NONDIFF) return DR_EINVAL;
    a.mode = mode; a.out = out_rgba; a.steps = steps;
    LitArgs q{};
    q.light = light;
    return launch_on(vol, launch_march_lit_fwd, a, q, (hipStream_t)stream);
}

int dr_march_lit_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                     int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                     const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W, int H,
                     int max_samples, float sampling_rate, const float *light, int mode, const float *grad_out,
                     const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                     float *d_tf, int64_t dtf_view_stride, double *d_light, float *d_light_ray, void *stream) {
    MarchArgs a;
    int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_,
                         rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!light || mode != DR_MODE_DIFF) return DR_EINVAL;
    rc = fill_bwd(a, grad_out, out_rgba, d_vol, dsx, dsy, dsz, dvol_view_stride, d_tf, dtf_view_stride);
    if (rc) return rc;
    if (!d_vol && !d_tf && !d_light && !d_light_ray) return 0;  // nothing requested
    LitArgs q{};
    q.light = light; q.d_light = d_light; q.d_light_ray = d_light_ray;
    return launch_on(vol, launch_march_lit_bwd, a, q, (hipStream_t)stream);
}

// what the RGBA-volume entries check before any HIP call, and the MarchArgs they share
static int fill_rgba(MarchArgs &a, RgbaArgs &q, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy,
                     int64_t sz, int64_t sc, int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_,
                     const float *rays, const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate) {
    const int rc = fill_rays(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                             W, H, max_samples, 1, sampling_rate, true);
    if (rc) return rc;
    q = RgbaArgs{};
    q.sc = sc;
    return 0;
}

int dr_march_rgba_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                      int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate, int mode,
                      float *out_rgba, int32_t *steps, void *stream) {
    MarchArgs a;
    RgbaArgs q;
    const int rc = fill_rgba(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, vol_view_stride, cam, entry, exit_, rays, nsamp,
                             n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_rgba) return DR_EINVAL;
    if (mode != DR_MODE_DIFF && mode != DR_MODE_NONDIFF) return DR_EINVAL;
    a.mode = mode; a.out = out_rgba; a.steps = steps;
    return launch_on(vol, launch_march_rgba_fwd, a, q, (hipStream_t)stream);
}

int dr_march_rgba_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                      int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                      const float *grad_out, const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz,
                      int64_t dsc, int64_t dvol_view_stride, void *stream) {
    MarchArgs a;
    RgbaArgs q;
    const int rc = fill_rgba(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, vol_view_stride, cam, entry, exit_, rays, nsamp,
                             n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!grad_out || !out_rgba) return DR_EINVAL;
    if (!d_vol) return 0;  // nothing requested
    a.mode = DR_MODE_DIFF;
    a.grad_out = grad_out; a.out_fwd = out_rgba;
    a.d_vol = d_vol; a.dsx = dsx; a.dsy = dsy; a.dsz = dsz; a.dvol_vs = dvol_view_stride;
    q.dsc = dsc;
    return launch_on(vol, launch_march_rgba_bwd, a, q, (hipStream_t)stream);
}

// dr_march_rgba_bwd_cam (pose null: d_cam [n_views][3]) and dr_march_rgba_bwd_pose (d_cam [n_views][10]): one implementation
static int march_rgba_bwd_camera(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                                 int64_t sc, int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_,
                                 const float *rays, const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                                 float sampling_rate, double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                                 const int32_t *steps, const float *grad_out, const float *out_rgba, const float *pose,
                                 const float *fov_v, double *d_cam, float *d_cam_ray, void *stream) {
    MarchArgs a;
    RgbaArgs q;
    CamArgs c;
    int rc = fill_rgba(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                       W, H, max_samples, sampling_rate);
    if (rc) return rc;
    rc = fill_camera(a, c, fov_rad, near_plane, jitter_seed, view_base, steps, grad_out, out_rgba, pose, fov_v, d_cam, d_cam_ray);
    if (rc) return rc;
    return launch_on(vol, launch_march_rgba_bwd_cam, a, q, c, (hipStream_t)stream);
}

int dr_march_rgba_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                          int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                          const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate, double fov_rad,
                          double near_plane, uint32_t jitter_seed, uint32_t view_base, const int32_t *steps,
                          const float *grad_out, const float *out_rgba, double *d_cam, float *d_cam_ray, void *stream) {
    return march_rgba_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, vol_view_stride, cam, entry, exit_, rays, nsamp,
                                 n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, jitter_seed, view_base, steps,
                                 grad_out, out_rgba, nullptr, nullptr, d_cam, d_cam_ray, stream);
}

int dr_march_rgba_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                           int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                           const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate, double fov_rad,
                           double near_plane, uint32_t jitter_seed, uint32_t view_base, const int32_t *steps,
                           const float *grad_out, const float *out_rgba, const float *pose, const float *fov_v, double *d_pose,
                           float *d_pose_ray, void *stream) {
    if (!pose) return DR_EINVAL;
    return march_rgba_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, vol_view_stride, cam, entry, exit_, rays, nsamp,
                                 n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, jitter_seed, view_base, steps,
                                 grad_out, out_rgba, pose, fov_v, d_pose, d_pose_ray, stream);
}

// what the depth entries check before any HIP call: fill_common with max_samples >= 1 and a finite rate; always differentiable
static int fill_depth(MarchArgs &a, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                      int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                      const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W, int H,
                      int max_samples, float sampling_rate) {
    const int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                               exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, 1, true);
    if (rc) return rc;
    a.mode = DR_MODE_DIFF;
    return 0;
}

int dr_march_depth_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                       int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                       const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W, int H,
                       int max_samples, float sampling_rate, float *out_moments, int32_t *steps, void *stream) {
    MarchArgs a;
    const int rc = fill_depth(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_,
                              rays, nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_moments) return DR_EINVAL;
    a.out = out_moments; a.steps = steps;
    return launch_on(vol, launch_march_depth_fwd, a, (hipStream_t)stream);
}

int dr_march_depth_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                       int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                       const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W, int H,
                       int max_samples, float sampling_rate, const float *grad_out, const float *out_moments, float *d_vol,
                       int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride, float *d_tf, int64_t dtf_view_stride,
                       void *stream) {
    MarchArgs a;
    int rc = fill_depth(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_, rays,
                        nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    rc = fill_bwd(a, grad_out, out_moments, d_vol, dsx, dsy, dsz, dvol_view_stride, d_tf, dtf_view_stride);
    if (rc) return rc;
    if (!d_vol && !d_tf) return 0;  // nothing requested
    return launch_on(vol, launch_march_depth_bwd, a, (hipStream_t)stream);
}

// dr_march_depth_bwd_cam (pose null: d_cam [n_views][3]) and dr_march_depth_bwd_pose (d_cam [n_views][10]): one implementation
static int march_depth_bwd_camera(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                                  int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                                  const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views,
                                  int W, int H, int max_samples, float sampling_rate, double fov_rad, double near_plane,
                                  uint32_t jitter_seed, uint32_t view_base, const int32_t *steps, const float *grad_out,
                                  const float *out_moments, const float *pose, const float *fov_v, double *d_cam,
                                  float *d_cam_ray, void *stream) {
    MarchArgs a;
    CamArgs c;
    int rc = fill_depth(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry, exit_, rays,
                        nsamp, n_views, W, H, max_samples, sampling_rate);
    if (rc) return rc;
    rc = fill_camera(a, c, fov_rad, near_plane, jitter_seed, view_base, steps, grad_out, out_moments, pose, fov_v, d_cam,
                     d_cam_ray);
    if (rc) return rc;
    return launch_on(vol, launch_march_depth_bwd_cam, a, c, (hipStream_t)stream);
}

int dr_march_depth_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                           int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                           const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                           int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, uint32_t jitter_seed,
                           uint32_t view_base, const int32_t *steps, const float *grad_out, const float *out_moments,
                           double *d_cam, float *d_cam_ray, void *stream) {
    return march_depth_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                                  exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, jitter_seed,
                                  view_base, steps, grad_out, out_moments, nullptr, nullptr, d_cam, d_cam_ray, stream);
}

int dr_march_depth_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                            int64_t vol_view_stride, const float *tf, int R, int64_t tf_view_stride, const float *cam,
                            const float *entry, const float *exit_, const float *rays, const int32_t *nsamp, int n_views, int W,
                            int H, int max_samples, float sampling_rate, double fov_rad, double near_plane, uint32_t jitter_seed,
                            uint32_t view_base, const int32_t *steps, const float *grad_out, const float *out_moments,
                            const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray, void *stream) {
    if (!pose) return DR_EINVAL;
    return march_depth_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, tf, R, tf_view_stride, cam, entry,
                                  exit_, rays, nsamp, n_views, W, H, max_samples, sampling_rate, fov_rad, near_plane, jitter_seed,
                                  view_base, steps, grad_out, out_moments, pose, fov_v, d_pose, d_pose_ray, stream);
}

// what the three projection entries check: fill_rays at the projections' fixed rate of 1 with max_samples >= 1, the mode, and
// arg_max for DR_PROJ_MAX
static int fill_proj(MarchArgs &a, ProjArgs &q, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy,
                     int64_t sz, int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_,
                     const float *rays, const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode,
                     const int32_t *arg_max) {
    const int rc = fill_rays(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                             W, H, max_samples, 1, 1.0f, false);
    if (rc) return rc;
    if (mode != DR_PROJ_SUM && mode != DR_PROJ_MAX) return DR_EINVAL;
    if (mode == DR_PROJ_MAX && !arg_max) return DR_EINVAL;
    q = ProjArgs{};
    q.mode = mode; q.variant = DR_VARIANT_AUTO; q.arg_max = const_cast<int32_t *>(arg_max);
    return 0;
}

int dr_project_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                   int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                   const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode, float *out, int32_t *arg_max,
                   void *stream) {
    MarchArgs a;
    ProjArgs q;
    int rc = fill_proj(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                       W, H, max_samples, mode, arg_max);
    if (rc) return rc;
    if (!out) return DR_EINVAL;
    a.out = out;
    return launch_on(vol, launch_project_fwd, a, q, (hipStream_t)stream);
}

int dr_project_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                   int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                   const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode, const float *grad_out,
                   const int32_t *arg_max, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                   int variant, void *stream) {
    MarchArgs a;
    ProjArgs q;
    int rc = fill_proj(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                       W, H, max_samples, mode, arg_max);
    if (rc) return rc;
    if (!grad_out) return DR_EINVAL;
    if (variant != DR_VARIANT_AUTO && variant != DR_VARIANT_BASELINE) return DR_EINVAL;
    if (!d_vol) return 0;  // nothing requested
    a.grad_out = grad_out; a.mode = DR_MODE_DIFF;
    a.d_vol = d_vol; a.dsx = dsx; a.dsy = dsy; a.dsz = dsz; a.dvol_vs = dvol_view_stride;
    q.variant = variant;
    return launch_on(vol, launch_project_bwd, a, q, (hipStream_t)stream);
}

// dr_project_bwd_cam (pose null) and dr_project_bwd_pose: one implementation
static int project_bwd_camera(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                              int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                              const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode, double fov_rad,
                              double near_plane, uint32_t jitter_seed, uint32_t view_base, const float *grad_out,
                              const int32_t *arg_max, const float *pose, const float *fov_v, double *d_cam, float *d_cam_ray,
                              void *stream) {
    MarchArgs a;
    ProjArgs q;
    int rc = fill_proj(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views,
                       W, H, max_samples, mode, arg_max);
    if (rc) return rc;
    if (!grad_out || !d_cam || !pose_fits(pose, fov_v)) return DR_EINVAL;
    if (!(near_plane > 0.0) || !(fov_rad > 0.0)) return DR_EINVAL;
    a.grad_out = grad_out; a.mode = DR_MODE_DIFF; a.fov_rad = fov_rad; a.near_plane = near_plane; a.pose = pose; a.fov_v = fov_v;
    q.jitter_seed = jitter_seed; q.view_base = view_base; q.d_cam = d_cam; q.d_cam_ray = d_cam_ray;
    return launch_on(vol, launch_project_bwd_cam, a, q, (hipStream_t)stream);
}

int dr_project_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                       int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                       const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode, double fov_rad,
                       double near_plane, uint32_t jitter_seed, uint32_t view_base, const float *grad_out,
                       const int32_t *arg_max, double *d_cam, float *d_cam_ray, void *stream) {
    return project_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views, W,
                              H, max_samples, mode, fov_rad, near_plane, jitter_seed, view_base, grad_out, arg_max, nullptr,
                              nullptr, d_cam, d_cam_ray, stream);
}

int dr_project_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                        int64_t vol_view_stride, const float *cam, const float *entry, const float *exit_, const float *rays,
                        const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode, double fov_rad,
                        double near_plane, uint32_t jitter_seed, uint32_t view_base, const float *grad_out,
                        const int32_t *arg_max, const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray,
                        void *stream) {
    if (!pose) return DR_EINVAL;
    return project_bwd_camera(vol, vol_dtype, VX, VY, VZ, sx, sy, sz, vol_view_stride, cam, entry, exit_, rays, nsamp, n_views, W,
                              H, max_samples, mode, fov_rad, near_plane, jitter_seed, view_base, grad_out, arg_max, pose, fov_v,
                              d_pose, d_pose_ray, stream);
}

// what the ray-bundle entries check of their ray count and t_near before any HIP call
static bool bundle_fits(int64_t N, float t_near) { return N > 0 && N < ((int64_t)1 << 31) && !std::isnan(t_near); }

int dr_bundle_setup(const float *origins, const float *dirs, int64_t N, int VX, int VY, int VZ, float sampling_rate, float t_near,
                    uint32_t jitter_seed, uint32_t ray_base, float *entry, float *exit_, int32_t *nsamp, void *stream) {
    if (!origins || !dirs || !entry || !exit_ || !nsamp) return DR_EINVAL;
    if (!bundle_fits(N, t_near) || VX < 2 || VY < 2 || VZ < 2 || !(sampling_rate > 0.0f)) return DR_EINVAL;
    BundleArgs b{};
    b.origins = origins; b.N = (int)N; b.t_near = t_near; b.jitter_seed = jitter_seed; b.ray_base = ray_base;
    return launch_on(entry, launch_bundle_setup, b, dirs, VX, VY, VZ, sampling_rate, entry, exit_, nsamp, (hipStream_t)stream);
}

// the three bundle marches: fill_common for one view of N x 1 rays whose camera rows are the origins, max_samples >= 1, a
// finite rate; always differentiable
static int fill_bundle(MarchArgs &a, BundleArgs &b, const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy,
                       int64_t sz, const float *tf, int R, const float *origins, const float *dirs, const float *entry,
                       const float *exit_, const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                       float t_near = 0.0f) {
    if (!bundle_fits(N, t_near)) return DR_EINVAL;
    const int rc = fill_common(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, 0, tf, R, 0, origins, entry, exit_, dirs, nsamp, 1,
                               (int)N, 1, max_samples, sampling_rate, 1, true);
    if (rc) return rc;
    a.mode = DR_MODE_DIFF;
    b = BundleArgs{};
    b.origins = origins; b.N = (int)N; b.t_near = t_near;
    return 0;
}

int dr_march_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                        const float *tf, int R, const float *origins, const float *dirs, const float *entry, const float *exit_,
                        const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate, float *out_rgba, int32_t *steps,
                        void *stream) {
    MarchArgs a;
    BundleArgs b;
    const int rc = fill_bundle(a, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, tf, R, origins, dirs, entry, exit_, nsamp, N,
                               max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_rgba) return DR_EINVAL;
    a.out = out_rgba; a.steps = steps;
    return launch_on(vol, launch_march_bundle_fwd, a, b, (hipStream_t)stream);
}

int dr_march_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                        const float *tf, int R, const float *origins, const float *dirs, const float *entry, const float *exit_,
                        const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate, const float *grad_out,
                        const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, float *d_tf, void *stream) {
    MarchArgs a;
    BundleArgs b;
    int rc = fill_bundle(a, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, tf, R, origins, dirs, entry, exit_, nsamp, N, max_samples,
                         sampling_rate);
    if (rc) return rc;
    rc = fill_bwd(a, grad_out, out_rgba, d_vol, dsx, dsy, dsz, 0, d_tf, 0);
    if (rc) return rc;
    if (!d_vol && !d_tf) return 0;  // nothing requested
    return launch_on(vol, launch_march_bundle_bwd, a, b, (hipStream_t)stream);
}

int dr_march_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                             const float *tf, int R, const float *origins, const float *dirs, const float *entry,
                             const float *exit_, const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                             const int32_t *steps, float t_near, uint32_t jitter_seed, uint32_t ray_base, const float *grad_out,
                             const float *out_rgba, float *d_origins, float *d_dirs, void *stream) {
    MarchArgs a;
    BundleArgs b;
    const int rc = fill_bundle(a, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, tf, R, origins, dirs, entry, exit_, nsamp, N,
                               max_samples, sampling_rate, t_near);
    if (rc) return rc;
    if (!steps || !grad_out || !out_rgba || !d_origins || !d_dirs) return DR_EINVAL;
    a.grad_out = grad_out; a.out_fwd = out_rgba;
    b.steps = steps; b.jitter_seed = jitter_seed; b.ray_base = ray_base; b.d_origins = d_origins; b.d_dirs = d_dirs;
    return launch_on(vol, launch_bundle_ray_grad, a, b, (hipStream_t)stream);
}

// the three bundle projections: fill_rays for one view of N x 1 rays whose camera rows are the origins, at the projections'
// fixed rate of 1 with max_samples >= 1; the mode, and arg_max for DR_PROJ_MAX
static int fill_proj_bundle(MarchArgs &a, BundleArgs &b, ProjArgs &q, const void *vol, int vol_dtype, int VX, int VY, int VZ,
                            int64_t sx, int64_t sy, int64_t sz, const float *origins, const float *dirs, const float *entry,
                            const float *exit_, const int32_t *nsamp, int64_t N, int max_samples, int mode, const int32_t *arg_max,
                            float t_near = 0.0f) {
    if (!bundle_fits(N, t_near)) return DR_EINVAL;
    const int rc = fill_rays(a, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, 0, origins, entry, exit_, dirs, nsamp, 1, (int)N, 1,
                             max_samples, 1, 1.0f, false);
    if (rc) return rc;
    if (mode != DR_PROJ_SUM && mode != DR_PROJ_MAX) return DR_EINVAL;
    if (mode == DR_PROJ_MAX && !arg_max) return DR_EINVAL;
    a.mode = DR_MODE_DIFF;
    b = BundleArgs{};
    b.origins = origins; b.N = (int)N; b.t_near = t_near;
    q = ProjArgs{};
    q.mode = mode; q.variant = DR_VARIANT_AUTO; q.arg_max = const_cast<int32_t *>(arg_max);
    return 0;
}

int dr_project_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                          const float *origins, const float *dirs, const float *entry, const float *exit_, const int32_t *nsamp,
                          int64_t N, int max_samples, int mode, float *out, int32_t *arg_max, void *stream) {
    MarchArgs a;
    BundleArgs b;
    ProjArgs q;
    const int rc = fill_proj_bundle(a, b, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, origins, dirs, entry, exit_, nsamp, N,
                                    max_samples, mode, arg_max);
    if (rc) return rc;
    if (!out) return DR_EINVAL;
    a.out = out;
    return launch_on(vol, launch_project_bundle_fwd, a, b, q, (hipStream_t)stream);
}

int dr_project_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                          const float *origins, const float *dirs, const float *entry, const float *exit_, const int32_t *nsamp,
                          int64_t N, int max_samples, int mode, const float *grad_out, const int32_t *arg_max, float *d_vol,
                          int64_t dsx, int64_t dsy, int64_t dsz, int variant, void *stream) {
    MarchArgs a;
    BundleArgs b;
    ProjArgs q;
    const int rc = fill_proj_bundle(a, b, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, origins, dirs, entry, exit_, nsamp, N,
                                    max_samples, mode, arg_max);
    if (rc) return rc;
    if (!grad_out) return DR_EINVAL;
    if (variant != DR_VARIANT_AUTO && variant != DR_VARIANT_BASELINE) return DR_EINVAL;
    if (!d_vol) return 0;  // nothing requested
    a.grad_out = grad_out;
    a.d_vol = d_vol; a.dsx = dsx; a.dsy = dsy; a.dsz = dsz;
    q.variant = variant;
    return launch_on(vol, launch_project_bundle_bwd, a, b, q, (hipStream_t)stream);
}

int dr_project_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                               const float *origins, const float *dirs, const float *entry, const float *exit_,
                               const int32_t *nsamp, int64_t N, int max_samples, int mode, float t_near, uint32_t jitter_seed,
                               uint32_t ray_base, const float *grad_out, const int32_t *arg_max, float *d_origins, float *d_dirs,
                               void *stream) {
    MarchArgs a;
    BundleArgs b;
    ProjArgs q;
    const int rc = fill_proj_bundle(a, b, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, origins, dirs, entry, exit_, nsamp, N,
                                    max_samples, mode, arg_max, t_near);
    if (rc) return rc;
    if (!grad_out || !d_origins || !d_dirs) return DR_EINVAL;
    a.grad_out = grad_out;
    b.jitter_seed = jitter_seed; b.ray_base = ray_base; b.d_origins = d_origins; b.d_dirs = d_dirs;
    return launch_on(vol, launch_project_bundle_ray_grad, a, b, q, (hipStream_t)stream);
}

// the three RGBA bundle marches: fill_rgba for one volume and one view of N x 1 rays whose camera rows are the
// origins (max_samples >= 1, a finite rate); always differentiable
static int fill_rgba_bundle(MarchArgs &a, RgbaArgs &q, BundleArgs &b, const void *vol, int vol_dtype, int VX, int VY, int VZ,
                            int64_t sx, int64_t sy, int64_t sz, int64_t sc, const float *origins, const float *dirs,
                            const float *entry, const float *exit_, const int32_t *nsamp, int64_t N, int max_samples,
                            float sampling_rate, float t_near = 0.0f) {
    if (!bundle_fits(N, t_near)) return DR_EINVAL;
    const int rc = fill_rgba(a, q, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, 0, origins, entry, exit_, dirs, nsamp, 1, (int)N, 1,
                             max_samples, sampling_rate);
    if (rc) return rc;
    a.mode = DR_MODE_DIFF;
    b = BundleArgs{};
    b.origins = origins; b.N = (int)N; b.t_near = t_near;
    return 0;
}

int dr_march_rgba_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                             const float *origins, const float *dirs, const float *entry, const float *exit_,
                             const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate, float *out_rgba,
                             int32_t *steps, void *stream) {
    MarchArgs a;
    RgbaArgs q;
    BundleArgs b;
    const int rc = fill_rgba_bundle(a, q, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, origins, dirs, entry, exit_, nsamp, N,
                                    max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_rgba) return DR_EINVAL;
    a.out = out_rgba; a.steps = steps;
    return launch_on(vol, launch_march_rgba_bundle_fwd, a, q, b, (hipStream_t)stream);
}

int dr_march_rgba_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                             const float *origins, const float *dirs, const float *entry, const float *exit_,
                             const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate, const float *grad_out,
                             const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dsc,
                             void *stream) {
    MarchArgs a;
    RgbaArgs q;
    BundleArgs b;
    const int rc = fill_rgba_bundle(a, q, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, origins, dirs, entry, exit_, nsamp, N,
                                    max_samples, sampling_rate);
    if (rc) return rc;
    if (!grad_out || !out_rgba) return DR_EINVAL;
    if (!d_vol) return 0;  // nothing requested
    a.grad_out = grad_out; a.out_fwd = out_rgba;
    a.d_vol = d_vol; a.dsx = dsx; a.dsy = dsy; a.dsz = dsz;
    q.dsc = dsc;
    return launch_on(vol, launch_march_rgba_bundle_bwd, a, q, b, (hipStream_t)stream);
}

int dr_march_rgba_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                                  int64_t sc, const float *origins, const float *dirs, const float *entry, const float *exit_,
                                  const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate, const int32_t *steps,
                                  float t_near, uint32_t jitter_seed, uint32_t ray_base, const float *grad_out,
                                  const float *out_rgba, float *d_origins, float *d_dirs, void *stream) {
    MarchArgs a;
    RgbaArgs q;
    BundleArgs b;
    const int rc = fill_rgba_bundle(a, q, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, sc, origins, dirs, entry, exit_, nsamp, N,
                                    max_samples, sampling_rate, t_near);
    if (rc) return rc;
    if (!steps || !grad_out || !out_rgba || !d_origins || !d_dirs) return DR_EINVAL;
    a.grad_out = grad_out; a.out_fwd = out_rgba;
    b.steps = steps; b.jitter_seed = jitter_seed; b.ray_base = ray_base; b.d_origins = d_origins; b.d_dirs = d_dirs;
    return launch_on(vol, launch_rgba_bundle_ray_grad, a, q, b, (hipStream_t)stream);
}

// the three depth bundle marches: fill_bundle's arguments and checks as they are; out_rgba holds the moments
int dr_march_depth_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                              const float *tf, int R, const float *origins, const float *dirs, const float *entry,
                              const float *exit_, const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                              float *out_rgba, int32_t *steps, void *stream) {
    MarchArgs a;
    BundleArgs b;
    const int rc = fill_bundle(a, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, tf, R, origins, dirs, entry, exit_, nsamp, N,
                               max_samples, sampling_rate);
    if (rc) return rc;
    if (!out_rgba) return DR_EINVAL;
    a.out = out_rgba; a.steps = steps;
    return launch_on(vol, launch_march_depth_bundle_fwd, a, b, (hipStream_t)stream);
}

int dr_march_depth_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                              const float *tf, int R, const float *origins, const float *dirs, const float *entry,
                              const float *exit_, const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                              const float *grad_out, const float *out_rgba, float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz,
                              float *d_tf, void *stream) {
    MarchArgs a;
    BundleArgs b;
    int rc = fill_bundle(a, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, tf, R, origins, dirs, entry, exit_, nsamp, N, max_samples,
                         sampling_rate);
    if (rc) return rc;
    rc = fill_bwd(a, grad_out, out_rgba, d_vol, dsx, dsy, dsz, 0, d_tf, 0);
    if (rc) return rc;
    if (!d_vol && !d_tf) return 0;  // nothing requested
    return launch_on(vol, launch_march_depth_bundle_bwd, a, b, (hipStream_t)stream);
}

int dr_march_depth_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ, int64_t sx, int64_t sy, int64_t sz,
                                   const float *tf, int R, const float *origins, const float *dirs, const float *entry,
                                   const float *exit_, const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                                   const int32_t *steps, float t_near, uint32_t jitter_seed, uint32_t ray_base,
                                   const float *grad_out, const float *out_rgba, float *d_origins, float *d_dirs, void *stream) {
    MarchArgs a;
    BundleArgs b;
    const int rc = fill_bundle(a, b, vol, vol_dtype, VX, VY, VZ, sx, sy, sz, tf, R, origins, dirs, entry, exit_, nsamp, N,
                               max_samples, sampling_rate, t_near);
    if (rc) return rc;
    if (!steps || !grad_out || !out_rgba || !d_origins || !d_dirs) return DR_EINVAL;
    a.grad_out = grad_out; a.out_fwd = out_rgba;
    b.steps = steps; b.jitter_seed = jitter_seed; b.ray_base = ray_base; b.d_origins = d_origins; b.d_dirs = d_dirs;
    return launch_on(vol, launch_depth_bundle_ray_grad, a, b, (hipStream_t)stream);
}

int dr_tf_momentum_step(float *tf, const float *d_tf, float *momentum, int n, float lr, float gamma, float max_grad,
                        void *stream) {
    if (!tf || !d_tf || !momentum || n <= 0 || !(max_grad >= 0.0f)) return DR_EINVAL;
    DeviceOf guard(tf);
    if (guard.err != hipSuccess) return (int)guard.err;
    return (int)launch_tf_momentum_step(tf, d_tf, momentum, n, lr, gamma, max_grad, (hipStream_t)stream);
}

}  // extern "C"
