// dr_kernels.h -- host-side launch entry points of the kernel translation units (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dr_experiment.h"

namespace dr {

// Everything a march launch needs; filled by capi.hip from the C-ABI arguments.
struct MarchArgs {
    const void *vol; int vol_dtype; int VX, VY, VZ; int64_t sx, sy, sz, vol_vs;
    const float *tf; int R; int64_t tf_vs;
    int RG; float g_scale;  // 2-D TF (march_tf2d.hip): [R][RG] texels, R its value rows; RG = 1 for the 1-D TF
    const float *cam, *entry, *exit_, *rays; const int32_t *nsamp;
    int n_views, W, H, S; float sr; int mode;
    int img_W, row0;  // the W rows of the buffers are rows [row0, row0 + W) of an image img_W rows wide (bands)
    float *out; int32_t *steps;
    // backward only
    const float *grad_out; const float *out_fwd;
    float *d_vol; int64_t dsx, dsy, dsz, dvol_vs;
    float *d_tf; int64_t dtf_vs;
    // brick path
    double fov_rad, near_plane;
    void *workspace; size_t workspace_bytes;
    int hints;                    // DR_HINT_* bits of the forward call
    // free camera; null: the fixed one (look at the origin, up = +y, the scalar fov_rad)
    const float *pose;            // [n_views][9] look_from, look_at, up; look_from equals cam
    const float *fov_v;           // [n_views] fov in radians, nullable: fov_rad for every view
};

// pose null: cam [n_views][3] and the fixed camera; else pose / fov_v as in MarchArgs, and cam is not read
hipError_t launch_ray_setup(const float *cam, const float *pose, const float *fov_v, int n_views, int W, int H, int img_W, int row0, int VX, int VY, int VZ,
                            double fov_rad, double near_plane, float sr, uint32_t jitter_seed, uint32_t view_base,
                            float *entry, float *exit_, float *rays, int32_t *nsamp, hipStream_t stream);

// Plain one-lane-per-ray kernels (DR_VARIANT_BASELINE): direct global gathers, global float atomics.
int launch_march_fwd_baseline(const MarchArgs &a, hipStream_t stream);
// The brick path's second backward pass (B2) runs the plain backward over the rays its forward flagged only; an empty filter: every ray.
struct RayFilter {
    const uint8_t *only_flagged = nullptr;   // [view][W][H]: march the rays whose flag is 1 ...
    const unsigned int *ws_mark = nullptr;   // ... unless *ws_mark != ws_mark_expect (the workspace is not this call's forward's: the
    unsigned int ws_mark_expect = 0;         //     flags are garbage, every ray is marched); may be null
    const unsigned int *ws_aux = nullptr;    // ... or *ws_aux != ws_aux_expect (the TF-only backward over the tape: the forward left no
    unsigned int ws_aux_expect = 0;          //     tape of this stride); may be null
};
int launch_march_bwd_baseline(const MarchArgs &a, const RayFilter &f, hipStream_t stream);

// Brick-centric kernels (DR_VARIANT_AUTO): LDS-staged bricks, per-(ray,layer) partial composites.
bool brick_path_supported(int VX, int VY, int VZ, int R);
bool brick_image_supported(int W, int H, int VX, int VY, int VZ);  // [layer][pixel] slot indices stay below 2^31
size_t brick_workspace_bytes(int n_views, int W, int H, int VX, int VY, int VZ);
int tape_stride_for(int VX, int VY, int VZ, float sr, int max_samples);   // samples per ray the DR_TAPE_TF tape reserves
size_t brick_workspace_bytes_tape(int n_views, int W, int H, int VX, int VY, int VZ, int max_samples, float sr);
bool flat_strides_ok(int64_t sx, int64_t sy, int64_t sz);  // 32-bit in-box offsets
// Word of the workspace header that says whose coarse tape the workspace holds (a fingerprint of the forward call that
// filled it, see ws_fingerprint); a forward served by the baseline kernels clears it (flat_invalidate_workspace).
constexpr int WS_MARK_WORD = 3;
hipError_t flat_invalidate_workspace(void *workspace, size_t workspace_bytes, hipStream_t stream);
int launch_march_fwd_flat(const MarchArgs &a, hipStream_t stream);   // one lane per sample
int launch_march_bwd_flat(const MarchArgs &a, hipStream_t stream);

// Camera gradient (camera_grad.hip): the extra arguments of dr_march_bwd_cam beside the MarchArgs of the backward
struct CamArgs {
    uint32_t jitter_seed, view_base;
    const int32_t *steps;   // the forward's live samples per ray
    double *d_cam;          // [n_views][3], accumulated ([n_views][10] with MarchArgs::pose: look_from, look_at, up, fov_rad)
    float *d_cam_ray;       // [n_views][W][H][3] per-ray contributions, nullable ([..][10] with MarchArgs::pose)
};
// weak: the C entry (capi.o) must load in a library linked from the other objects alone (tests/test_abi.py's what-if build)
__attribute__((weak)) int launch_camera_grad(const MarchArgs &a, const CamArgs &c, hipStream_t stream);

// The image losses: what dr_dssim_mse_fwd / _bwd and dr_msssim_mse_fwd / _bwd both take (checked and copied once, capi.hip)
struct ImageArgs {
    const float *x, *y;
    int N, C, H, W;
    int64_t strides[4];        // element strides of the logical NCHW, shared by x, y and the gradients
    double data_range, win_sigma, K1, K2;
    int win_size;
    double *stats;             // the forward writes, the backward reads
    const float *upstream;     // backward: (d loss, d dssim or d dms, d mse) on the device, nullable = (1, 0, 0)
    float *grad_x, *grad_y;    // backward; grad_y nullable
};
// DSSIM + MSE image loss (image_loss.hip); stats: [N*C] S_nc, then loss, dssim, mse
struct LossArgs : ImageArgs {
    int flags;                 // DR_SSIM_NONNEGATIVE
};
// weak, as launch_camera_grad: capi.o must load in a library linked without image_loss.o
__attribute__((weak)) int launch_dssim_mse_fwd(const LossArgs &a, hipStream_t stream);
__attribute__((weak)) int launch_dssim_mse_bwd(const LossArgs &a, hipStream_t stream);

// MS-SSIM + MSE image loss (msssim.hip): the arguments of dr_msssim_mse_fwd / dr_msssim_mse_bwd
constexpr int MS_MAX_LEVELS = 5;   // DR_MSSSIM_MAX_LEVELS of the public header (checked in capi.hip)
struct MSArgs : ImageArgs {   // stats: v[levels][N*C], ms[N*C], loss, dms, mse
    double weights[MS_MAX_LEVELS];
    int levels;
    void *workspace;           // msssim_layout(...).bytes
};
// The workspace: levels 1..L-1 of X and Y (pyramid), and for the backward dX_l (and dY_l), each a dense [N*C][H_l][W_l] f32
// block at a 256-byte aligned offset. H_{l+1} = ceil(H_l / 2) (avg_pool2d(2, padding=H_l % 2)).
struct MSLayout {
    int H[MS_MAX_LEVELS], W[MS_MAX_LEVELS];
    size_t x[MS_MAX_LEVELS], y[MS_MAX_LEVELS], dx[MS_MAX_LEVELS], dy[MS_MAX_LEVELS];
    size_t bytes;
};
inline MSLayout msssim_layout(int N, int C, int H, int W, int levels, bool want_grad_y) {
    MSLayout m{};
    size_t off = 0;
    auto take = [&off](size_t n) { const size_t o = off; off += (n * sizeof(float) + 255) / 256 * 256; return o; };
    for (int l = 0; l < levels; ++l) {
        m.H[l] = l == 0 ? H : (m.H[l - 1] + 1) / 2;
        m.W[l] = l == 0 ? W : (m.W[l - 1] + 1) / 2;
        if (l == 0) continue;
        const size_t n = (size_t)N * C * m.H[l] * m.W[l];
        m.x[l] = take(n);
        m.y[l] = take(n);
        m.dx[l] = take(n);
        if (want_grad_y) m.dy[l] = take(n);
    }
    m.bytes = off;
    return m;
}
// weak, as launch_camera_grad: capi.o must load in a library linked without msssim.o
__attribute__((weak)) int launch_msssim_mse_fwd(const MSArgs &a, hipStream_t stream);
__attribute__((weak)) int launch_msssim_mse_bwd(const MSArgs &a, hipStream_t stream);

// 3-D total variation (tv_loss.hip): the arguments of dr_tv3d_fwd / dr_tv3d_bwd
struct TVArgs {
    const void *vol;
    int vol_dtype, B, D, H, W;
    int64_t strides[4];        // element strides of the logical (B, D, H, W)
    int norm;                  // DR_TV_*
    double eps;
    double *sum;               // forward: written
    const float *upstream;     // backward: d objective / d sum on the device, nullable = 1
    float scale;
    float *grad;               // backward
    int64_t grad_strides[4];
    int accumulate;
};
// weak, as launch_camera_grad: capi.o must load in a library linked without tv_loss.o
__attribute__((weak)) int launch_tv3d_fwd(const TVArgs &a, hipStream_t stream);
__attribute__((weak)) int launch_tv3d_bwd(const TVArgs &a, hipStream_t stream);

// March with a 2-D (value, gradient-magnitude) transfer function (march_tf2d.hip): dr_march_tf2d_fwd / _bwd.
// weak, as launch_camera_grad: capi.o must load in a library linked without march_tf2d.o
__attribute__((weak)) int launch_march_tf2d_fwd(const MarchArgs &a, hipStream_t stream);
__attribute__((weak)) int launch_march_tf2d_bwd(const MarchArgs &a, hipStream_t stream);

// X-ray line-integral and maximum-intensity projections (projection.hip): the arguments of dr_project_fwd /
// _bwd / _bwd_cam beside their MarchArgs (volume, ray buffers, extents, max_samples S; the camera's fov_rad / near_plane; the
// backward's d_vol and grad_out, a [view][W][H] f32 image)
struct ProjArgs {
    int mode, variant;                 // DR_PROJ_*; DR_VARIANT_AUTO (windowed SUM backward) or DR_VARIANT_BASELINE
    int32_t *arg_max;                  // MAX: [view][W][H], written by the forward, read by the backwards
    uint32_t jitter_seed, view_base;   // camera backward
    double *d_cam;                     // [n_views][3], accumulated ([n_views][10] with MarchArgs::pose)
    float *d_cam_ray;                  // [n_views][W][H][3] per-ray contributions, nullable ([..][10] with MarchArgs::pose)
};
// weak, as launch_camera_grad: capi.o must load in a library linked without projection.o
__attribute__((weak)) int launch_project_fwd(const MarchArgs &a, const ProjArgs &q, hipStream_t stream);
__attribute__((weak)) int launch_project_bwd(const MarchArgs &a, const ProjArgs &q, hipStream_t stream);
__attribute__((weak)) int launch_project_bwd_cam(const MarchArgs &a, const ProjArgs &q, hipStream_t stream);

// March through a pre-classified RGBA volume (march_rgba.hip): what dr_march_rgba_fwd / _bwd take beside their
// MarchArgs (volume and its x/y/z and view strides, ray buffers, extents, max_samples S, sr, mode; the backward's grad_out,
// out_fwd and d_vol with its strides): the channel strides of the volume and of d_vol, in elements
struct RgbaArgs {
    int64_t sc, dsc;
};
// weak, as launch_camera_grad: capi.o must load in a library linked without march_rgba.o
__attribute__((weak)) int launch_march_rgba_fwd(const MarchArgs &a, const RgbaArgs &q, hipStream_t stream);
__attribute__((weak)) int launch_march_rgba_bwd(const MarchArgs &a, const RgbaArgs &q, hipStream_t stream);
// ... and its camera gradient: dr_march_rgba_bwd_cam / _bwd_pose, CamArgs as for launch_camera_grad
__attribute__((weak)) int launch_march_rgba_bwd_cam(const MarchArgs &a, const RgbaArgs &q, const CamArgs &c, hipStream_t stream);

// March with a free light and Phong material (march_lit.hip): what dr_march_lit_fwd / _bwd take beside their
// MarchArgs (the 1-D march's, without workspace, variant or bands)
struct LitArgs {
    const float *light;      // [n_views][10]: position, colour, ambient, diffuse, specular, shininess
    double *d_light;         // backward: [n_views][10], accumulated, nullable
    float *d_light_ray;      // backward: [n_views][W][H][10] per-ray contributions, overwritten, nullable
};
// weak, as launch_camera_grad: capi.o must load in a library linked without march_lit.o
__attribute__((weak)) int launch_march_lit_fwd(const MarchArgs &a, const LitArgs &q, hipStream_t stream);
__attribute__((weak)) int launch_march_lit_bwd(const MarchArgs &a, const LitArgs &q, hipStream_t stream);

// Ray-depth moments of the differentiable march (march_depth.hip): dr_march_depth_fwd / _bwd take the 1-D
// march's MarchArgs (no workspace, variant, mode or bands); _bwd_cam / _bwd_pose CamArgs as launch_camera_grad.
// weak, as launch_camera_grad: capi.o must load in a library linked without march_depth.o
__attribute__((weak)) int launch_march_depth_fwd(const MarchArgs &a, hipStream_t stream);
__attribute__((weak)) int launch_march_depth_bwd(const MarchArgs &a, hipStream_t stream);
__attribute__((weak)) int launch_march_depth_bwd_cam(const MarchArgs &a, const CamArgs &c, hipStream_t stream);

// The differentiable 1-D TF march over a bundle of rays (march_bundle.hip): what dr_bundle_setup and
// dr_march_bundle_fwd / _bwd / _bwd_rays take beside their MarchArgs (the 1-D march's with n_views = 1, W = N, H = 1, cam the
// origins and rays the directions; no workspace, variant, mode or bands)
struct BundleArgs {
    const float *origins;              // [N][3]
    int N;
    float t_near;                      // -INFINITY: off
    uint32_t jitter_seed, ray_base;    // setup and ray gradient
    const int32_t *steps;              // ray gradient: the forward's live samples per ray
    float *d_origins, *d_dirs;         // ray gradient: [N][3] each, overwritten
};
// weak, as launch_camera_grad: capi.o must load in a library linked without march_bundle.o
__attribute__((weak)) int launch_bundle_setup(const BundleArgs &b, const float *dirs, int VX, int VY, int VZ, float sr, float *entry,
                                              float *exit_, int32_t *nsamp, hipStream_t stream);
__attribute__((weak)) int launch_march_bundle_fwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream);
__attribute__((weak)) int launch_march_bundle_bwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream);
__attribute__((weak)) int launch_bundle_ray_grad(const MarchArgs &a, const BundleArgs &b, hipStream_t stream);

// The projections over a bundle of rays (projection_bundle.hip): dr_project_bundle_fwd / _bwd / _bwd_rays take the
// bundle's MarchArgs without a table (n_views = 1, W = N, H = 1, cam the origins, rays the directions), its BundleArgs (no
// steps) and the projections' ProjArgs (mode, variant, arg_max [N]; grad_out is an [N] f32 vector)
// weak, as launch_camera_grad: capi.o must load in a library linked without projection_bundle.o
__attribute__((weak)) int launch_project_bundle_fwd(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream);
__attribute__((weak)) int launch_project_bundle_bwd(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream);
__attribute__((weak)) int launch_project_bundle_ray_grad(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream);

// The RGBA march over a bundle of rays (march_rgba_bundle.hip): dr_march_rgba_bundle_fwd / _bwd / _bwd_rays take
// the bundle's MarchArgs without a table (n_views = 1, W = N, H = 1, cam the origins, rays the directions; one volume, no view
// strides), the RGBA march's RgbaArgs and the bundle's BundleArgs
// weak, as launch_camera_grad: capi.o must load in a library linked without march_rgba_bundle.o
__attribute__((weak)) int launch_march_rgba_bundle_fwd(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream);
__attribute__((weak)) int launch_march_rgba_bundle_bwd(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream);
__attribute__((weak)) int launch_rgba_bundle_ray_grad(const MarchArgs &a, const RgbaArgs &q, const BundleArgs &b, hipStream_t stream);

// The depth march over a bundle of rays (march_depth_bundle.hip): dr_march_depth_bundle_fwd / _bwd / _bwd_rays take
// the bundle's MarchArgs and BundleArgs exactly as launch_march_bundle_fwd / _bwd / launch_bundle_ray_grad do; `out` holds the
// moments [N][4] = (M1, M2, 0, A), and only the alpha column of d_tf is written
// weak, as launch_camera_grad: capi.o must load in a library linked without march_depth_bundle.o
__attribute__((weak)) int launch_march_depth_bundle_fwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream);
__attribute__((weak)) int launch_march_depth_bundle_bwd(const MarchArgs &a, const BundleArgs &b, hipStream_t stream);
__attribute__((weak)) int launch_depth_bundle_ray_grad(const MarchArgs &a, const BundleArgs &b, hipStream_t stream);

// Loss / optimiser epilogue (epilogue.hip)
hipError_t launch_mse_loss_grad(const float *out, const float *ref, int64_t n, float inv_norm, float *grad,
                                double *loss, hipStream_t stream);
hipError_t launch_tf_momentum_step(float *tf, const float *g, float *mom, int n, float lr, float gamma,
                                   float max_grad, hipStream_t stream);

}  // namespace dr
