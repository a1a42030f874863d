// march_rgba.hip -- the march through a pre-classified RGBA volume, for gfx950.
// The shape of march_baseline.hip / march_tf2d.hip: one lane per ray, a wave per 8x8 pixel tile, 256-thread workgroups, direct
// global gathers, the sequential float32 recurrence and the tape-free adjoint (suffix = out - prefix). There is no table and no
// shading: a sample is the trilinear interpolation of the volume's four channels (one cell, eight corners, x -> y -> z through
// mixf, per channel), its opacity opacity_of_alpha(a, 1/sr), and it composites with L = 1.
//   VEC: the channels of a voxel are neighbours in memory and every voxel is 16-B (f32) / 8-B (f16) aligned: a corner is ONE
//   load instead of four. The host decides once per launch (rgba_vec_ok); both paths read the same values and do the same
//   arithmetic in the same order, so their images are the same bits.
// The camera gradient of the march is the third kernel here: D8's four per-ray sums (camera_grad.hip) with the
// per-sample part of a four-channel volume, and dr_camera.h's once-per-ray tails and reductions.
#include "dr_camera.h"
#include "dr_rgba.h"

namespace dr {

// The 4-channel view: the scalar kernels' view (extents, x/y/z strides, the cell scale) plus the channel stride.
template <typename VT>
struct RgbaParams {
    VolView<VT> vol; int64_t sc, vol_vs;
    const float *cam, *entry, *exit_, *rays; const int32_t *nsamp;
    int W, H, S; float inv_sr;
    float *out; int32_t *steps;
    const float *grad_out, *out_fwd;
    GradView dvol; int64_t dsc, dvol_vs;
};

template <typename VT>
static inline RgbaParams<VT> make_rgba_params(const MarchArgs &a, const RgbaArgs &q) {
    RgbaParams<VT> P;
    P.vol = make_vol_view<VT>(a); P.sc = q.sc; P.vol_vs = a.vol_vs;
    P.cam = a.cam; P.entry = a.entry; P.exit_ = a.exit_; P.rays = a.rays; P.nsamp = a.nsamp;
    P.W = a.W; P.H = a.H; P.S = a.S; P.inv_sr = 1.0f / a.sr;
    P.out = a.out; P.steps = a.steps;
    P.grad_out = a.grad_out; P.out_fwd = a.out_fwd;
    P.dvol.p = a.d_vol; P.dvol.sx = a.dsx; P.dvol.sy = a.dsy; P.dvol.sz = a.dsz; P.dsc = q.dsc; P.dvol_vs = a.dvol_vs;
    return P;
}

template <typename VT, bool VEC, bool NONDIFF>
__global__ __launch_bounds__(256) void march_rgba_fwd_kernel(RgbaParams<VT> P) {
    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const int view = blockIdx.y;
    const size_t p = ray_index(P.W, P.H, view, i, j);
    Ray<VT> ray;
    open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
    const VolView<VT> &vol = ray.vol;
    const int m = rgba_samples(ray.rg.n, P.S, NONDIFF);

    Composite c;
    int cnt = 0;
    for (int s = 0; s < m; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        Cell cell;
        tri_cell(vol, sm.px, sm.py, sm.pz, cell);
        const float4 v = tri_sample4<VT, VEC>(vol, P.sc, cell);
        ++cnt;
        if (NONDIFF && !(v.w > 1e-3f)) continue;
        sm.r = v.x; sm.g = v.y; sm.b = v.z; sm.a = v.w; sm.L = 1.0f;
        sm.op = opacity_of_alpha(sm.a, P.inv_sr);
        c.add(sm);
    }
    reinterpret_cast<float4 *>(P.out)[p] = c.pixel(NONDIFF);
    if (P.steps) P.steps[p] = cnt;
}

template <typename VT, bool VEC>
__global__ __launch_bounds__(256) void march_rgba_bwd_kernel(RgbaParams<VT> P) {
    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const int view = blockIdx.y;
    const size_t p = ray_index(P.W, P.H, view, i, j);
    GradView dv = P.dvol;
    Ray<VT> ray;
    open_ray<true>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp, P.grad_out, P.out_fwd, &dv, P.dvol_vs);
    const VolView<VT> &vol = ray.vol;
    const int m = rgba_samples(ray.rg.n, P.S, false);

    Composite c;
    VoxelRun run;
    for (int s = 0; s < m; ++s) {
        if (!(c.A < 0.99f)) break;
        Sample sm;
        sample_pos(ray, s, sm.px, sm.py, sm.pz);
        Cell cell;
        tri_cell(vol, sm.px, sm.py, sm.pz, cell);
        const float4 v = tri_sample4<VT, VEC>(vol, P.sc, cell);
        sm.r = v.x; sm.g = v.y; sm.b = v.z; sm.a = v.w;
        sm.L = sm.Lraw = 1.0f; sm.flat = true;   // no shading: sample_adjoint's normal path is off
        sm.op = opacity_of_alpha(sm.a, P.inv_sr);
        const float T = c.add(sm);
        const bool last = (s == m - 1) || !(c.A < 0.99f);
        SampleAdj ad;
        sample_adjoint(sm, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);
        const float adj[4] = {ad.r_bar, ad.g_bar, ad.b_bar, ad.a_bar};
        if (!run.same(cell)) { run.flush(dv, P.dsc, vol.VX, vol.VY, vol.VZ); run.start(cell); }
        run.add(cell, adj);
    }
    run.flush(dv, P.dsc, vol.VX, vol.VY, vol.VZ);
}

// What the camera gradient reads beside the march's parameters (camera_grad.hip's CamParams; no row bands: the buffers are the
// whole image)
template <typename VT>
struct RgbaCamParams : RgbaParams<VT> {
    const int32_t *fwd_steps;   // the forward's live samples per ray
    CamFields cf;               // (aspect: W / H)
};

// Gradient of the differentiable RGBA march w.r.t. look_from ([views][3]) or, POSE, the free camera's ten parameters
// (DESIGN.md D16). camera_grad_kernel's shape and frozen branches (n, the live samples, the jitter draw, the slab faces, the
// cells); per sample P_s = dL/dpos_s = sum over the channels of the channel's adjoint times its slopes. There is no lighting,
// so D8's H_s = D_s = 0 and G_s = P_s: four f32 sums per ray, the tail once per ray, f64 per workgroup.
template <typename VT, bool VEC, bool POSE>
__global__ __launch_bounds__(256) void march_rgba_cam_kernel(RgbaCamParams<VT> P) {
    __shared__ double red[3][256];
    const int view = blockIdx.y;
    f3 dcam = make_f3(0.f, 0.f, 0.f);
    PoseGrad dpose = pose_zero();
    int i, j;
    const bool in_img = tile_pixel(P.W, P.H, i, j);
    const size_t p = ray_index(P.W, P.H, view, i, j);
    // H6: a single-sample ray sits at 0/0 in the reference and contributes nothing
    if (in_img && P.nsamp[p] > 1) {
        Ray<VT> ray;
        open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
        const VolView<VT> &vol = ray.vol;
        const RayGeom &rg = ray.rg;
        const f3 lf = ray.cam, vd = ray.vd;
        const int m = min(rgba_samples(rg.n, P.S, false), P.fwd_steps[p]);   // the forward's live samples (early termination frozen)
        open_adjoint(ray, p, P.grad_out, P.out_fwd);
        f3 sP = make_f3(0.f, 0.f, 0.f), sTP = make_f3(0.f, 0.f, 0.f);
        float s0 = 0.f, s1 = 0.f;
        Composite c;
        for (int s = 0; s < m; ++s) {
            Sample sm;
            sample_pos(ray, s, sm.px, sm.py, sm.pz);
            Cell cell;
            tri_cell(vol, sm.px, sm.py, sm.pz, cell);
            float4 gx, gy, gz;
            const float4 v = tri_sample4_grad<VT, VEC>(vol, P.sc, cell, sm.px, sm.py, sm.pz, gx, gy, gz);
            sm.r = v.x; sm.g = v.y; sm.b = v.z; sm.a = v.w;
            sm.L = sm.Lraw = 1.0f; sm.flat = true;   // no shading, as march_rgba_bwd_kernel
            sm.op = opacity_of_alpha(sm.a, P.inv_sr);
            const float T = c.add(sm);
            const bool last = s == m - 1;
            SampleAdj ad;
            sample_adjoint(sm, ray.vd, T, c.suffix(ray.go, ray.of), last, ray.go, P.inv_sr, ad);
            const f3 Ps = make_f3(ad.r_bar * gx.x + ad.g_bar * gx.y + ad.b_bar * gx.z + ad.a_bar * gx.w,
                                  ad.r_bar * gy.x + ad.g_bar * gy.y + ad.b_bar * gy.z + ad.a_bar * gy.w,
                                  ad.r_bar * gz.x + ad.g_bar * gz.y + ad.b_bar * gz.z + ad.a_bar * gz.w);
            const float f = (float)s / (float)(rg.n - 1);
            const float t = mixf(rg.t0, rg.exit_, f);
            const float gv = dot3(Ps, vd);
            sP = f3_add(sP, Ps);
            sTP = f3_fma(t, Ps, sTP);
            s0 = fmaf(1.0f - f, gv, s0);
            s1 = fmaf(f, gv, s1);
        }

        if (POSE) {
            // once per ray: the ten pose gradients from the four sums (dr_camera.h), then D5
            const PoseRay q = pose_ray(P.cf.pose, P.cf.fov_v, view, P.cf.near_d, P.cf.aspect, P.cf.near_w, P.cf.near_h, i, P.W, j,
                                       P.H, rg.n, P.cf.jitter_seed, P.cf.view_base + (uint32_t)view);
            dpose = pose_finite(pose_ray_grad(lf, q, vd, P.cf.near_, sP, sTP, s0 * q.A, fmaf(s0, 1.0f - q.A, s1)));
        } else {
            // once per ray: J_vd, the rows of the slab faces the forward picked and the jitter draw behind grad t0
            M3 J;
            f3 g_tmin, g_tmax, g_t0;
            float u;
            camera_ray_tail(lf, vd, i, P.W, j, P.H, P.cf.near_, P.cf.near_w, P.cf.near_h, rg.n, P.cf.jitter_seed,
                            P.cf.view_base + (uint32_t)view, J, g_tmin, g_tmax, g_t0, u);
            dcam = f3_add(sP, mul_t(J, sTP));
            dcam = f3_fma(s0, g_t0, dcam);
            dcam = f3_fma(s1, g_tmax, dcam);
            // D5: a NaN ray (NaN upstream gradient or pixel) contributes nothing, infinities are clamped
            dcam = make_f3(finite_or_zero(dcam.x), finite_or_zero(dcam.y), finite_or_zero(dcam.z));
        }
    }
    if (POSE) pose_reduce(dpose, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
    else camera_reduce(dcam, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
}

template <typename VT>
static int rgba_fwd_dispatch(const MarchArgs &a, const RgbaArgs &q, hipStream_t stream) {
    const RgbaParams<VT> P = make_rgba_params<VT>(a, q);
    const bool vec = rgba_vec_ok(a, q);
    if (a.mode == DR_MODE_DIFF)
        return launch_tiles(vec ? march_rgba_fwd_kernel<VT, true, false> : march_rgba_fwd_kernel<VT, false, false>, a, 0, stream, P);
    return launch_tiles(vec ? march_rgba_fwd_kernel<VT, true, true> : march_rgba_fwd_kernel<VT, false, true>, a, 0, stream, P);
}

template <typename VT>
static int rgba_bwd_dispatch(const MarchArgs &a, const RgbaArgs &q, hipStream_t stream) {
    const RgbaParams<VT> P = make_rgba_params<VT>(a, q);
    return launch_tiles(rgba_vec_ok(a, q) ? march_rgba_bwd_kernel<VT, true> : march_rgba_bwd_kernel<VT, false>, a, 0, stream, P);
}

int launch_march_rgba_fwd(const MarchArgs &a, const RgbaArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? rgba_fwd_dispatch<__half>(a, q, stream) : rgba_fwd_dispatch<float>(a, q, stream);
}

int launch_march_rgba_bwd(const MarchArgs &a, const RgbaArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? rgba_bwd_dispatch<__half>(a, q, stream) : rgba_bwd_dispatch<float>(a, q, stream);
}

template <typename VT, bool POSE>
static int rgba_cam_dispatch(const MarchArgs &a, const RgbaArgs &q, const CamArgs &c, hipStream_t stream) {
    RgbaCamParams<VT> P{make_rgba_params<VT>(a, q)};
    P.fwd_steps = c.steps;
    P.cf = fill_cam_fields(a, c.jitter_seed, c.view_base, c.d_cam, c.d_cam_ray);
    return launch_tiles(rgba_vec_ok(a, q) ? march_rgba_cam_kernel<VT, true, POSE> : march_rgba_cam_kernel<VT, false, POSE>, a, 0,
                        stream, P);
}

// MarchArgs::pose null: d look_from into c.d_cam [n_views][3]; else the ten pose gradients into [n_views][10]
int launch_march_rgba_bwd_cam(const MarchArgs &a, const RgbaArgs &q, const CamArgs &c, hipStream_t stream) {
    if (a.pose)
        return a.vol_dtype == DR_F16 ? rgba_cam_dispatch<__half, true>(a, q, c, stream) : rgba_cam_dispatch<float, true>(a, q, c, stream);
    return a.vol_dtype == DR_F16 ? rgba_cam_dispatch<__half, false>(a, q, c, stream) : rgba_cam_dispatch<float, false>(a, q, c, stream);
}

}  // namespace dr
