// projection_bundle.hip -- X-ray line-integral (DR_PROJ_SUM) and maximum-intensity (DR_PROJ_MAX) projections of an arbitrary
// bundle of rays, with gradients to the volume and to every ray's origin and direction, for gfx950.
//
// A ray is an input, as in march_bundle.hip (D19): origins [N][3] and unit directions [N][3], ray buffers from dr_bundle_setup.
// The per-sample work is projection.hip's (D13), statement for statement, with the lane's own origin where those kernels read
// the view's camera: the rays of a pinhole view give that view's projection, bit for bit.
//   s < m = min(n, S) (0 for n <= 1), pos_s = o + mix(t0, exit, s/(n-1)) d;
//   SUM: out = D sum_s mu(pos_s), D = (exit - entry) / n;   MAX: the first maximum by a strict >, its index in arg_max (-1: none).
// Shape: dr_bundle.h's -- one lane per ray, 256-lane workgroups over the linear ray index.
#include "dr_bundle.h"
#include "dr_camera.h"
#include "dr_wave.h"

namespace dr {

template <typename VT>
struct ProjBundleParams : RayParams<VT> {   // (cam: the origins [N][3]; rays: the directions [N][3]; W = N, H = 1)
    int N;
    int32_t *arg_max;                   // MAX: the forward writes it, the backwards read it
    float win_t0, win_tmin;             // windowed backward: the first and the shallowest window depth, in t
    float t_near;
    uint32_t jitter_seed, ray_base;
    float *d_origins, *d_dirs;
};

// samples of a ray and the sample spacing, as projection.hip's proj_samples / proj_delta
__device__ __forceinline__ int bundle_proj_samples(int n, int S) { return n > 1 ? min(n, S) : 0; }
__device__ __forceinline__ float bundle_proj_delta(const RayGeom &rg) { return (rg.exit_ - rg.entry) / (float)rg.n; }

// project_fwd_kernel per ray
template <typename VT, int MODE>
__global__ __launch_bounds__(256) void project_bundle_fwd_kernel(ProjBundleParams<VT> P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    Ray<VT> ray;
    open_bundle_ray<false>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
    const VolView<VT> &vol = ray.vol;
    const RayGeom &rg = ray.rg;
    const int m = bundle_proj_samples(rg.n, P.S);
    if (MODE == DR_PROJ_SUM) {
        float acc = 0.0f;
        for (int s = 0; s < m; ++s) {
            float px, py, pz;
            sample_pos(ray, s, px, py, pz);
            acc += tri_sample(vol, px, py, pz);
        }
        P.out[p] = m > 0 ? bundle_proj_delta(rg) * acc : 0.0f;
    } else {
        float best = 0.0f;
        int arg = -1;
        for (int s = 0; s < m; ++s) {
            float px, py, pz;
            sample_pos(ray, s, px, py, pz);
            const float v = tri_sample(vol, px, py, pz);
            if (arg < 0 || v > best) { best = v; arg = s; }
        }
        P.out[p] = best;
        P.arg_max[p] = arg;
    }
}

// project_bwd_plain_kernel per ray: global float atomics per tap; SUM (every sample, weight g D: DR_VARIANT_BASELINE and the
// yardstick of the windowed kernel) and MAX (the one stored argmax sample, weight g)
template <typename VT, int MODE>
__global__ __launch_bounds__(256) void project_bundle_bwd_plain_kernel(ProjBundleParams<VT> P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    const VolView<VT> vol = P.vol;
    const GradView dv = P.dvol;
    const f3 o = load_f3(P.cam, p);
    RayGeom rg;
    load_ray(P.entry, P.exit_, P.rays, P.nsamp, p, rg);
    const int m = bundle_proj_samples(rg.n, P.S);
    if (MODE == DR_PROJ_SUM) {
        const float gd = m > 0 ? finite_or_zero(P.grad_out[p] * bundle_proj_delta(rg)) : 0.0f;
        if (gd == 0.0f) return;
        for (int s = 0; s < m; ++s) {
            float px, py, pz;
            sample_pos(rg, o.x, o.y, o.z, s, px, py, pz);
            tri_scatter_global(vol, dv, px, py, pz, gd);
        }
    } else {
        const int s = P.arg_max[p];
        const float g = finite_or_zero(P.grad_out[p]);
        if (s < 0 || s >= m || g == 0.0f) return;
        float px, py, pz;
        sample_pos(rg, o.x, o.y, o.z, s, px, py, pz);
        tri_scatter_global(vol, dv, px, py, pz, g);
    }
}

// Windowed SUM backward: project_bwd_window_kernel with the workgroup's pixel tile replaced by a group of PBW_GROUP consecutive
// rays, each lane holding its own origin. The group walks its rays front to back through depth windows of t; per window every
// lane takes its samples with t_s below the window's far end, the group bounds the cells they touch by the cells of each lane's
// first and last sample in the window, adds g D w_tap into that box in LDS (ds_add_f32; a tap outside the box goes to global
// memory) and then adds the box to d_vol with global float atomics in the order of d_vol's contiguous axis. A box above the LDS
// budget halves the window, down to PBW_MIN_VOX voxels deep.
// One departure, for incoherent bundles: a group whose box does not fit even at the shallowest window is not a tile of
// neighbouring rays, and its next window would fit no better -- it finishes ALL remaining samples of its rays with per-tap
// global atomics in one go, as the plain kernel, instead of paying two barriers and six reductions per two-voxel window.
// Whether a group of 256 rays is coherent is the caller's ray order (bundle.tile_order for an image's rays).
constexpr int PBW_GROUP = 256;        // rays of a group: the workgroup
constexpr int PBW_BOX = 7680;         // LDS floats of the box: 30 KiB, five workgroups (20 waves) per CU by LDS
constexpr float PBW_WIN_VOX = 16.0f;  // first window depth, in voxels of the finest axis
constexpr float PBW_MIN_VOX = 2.0f;   // shallowest window before the group falls through to global atomics
static_assert(PBW_GROUP == 256, "a group is dr_bundle.h's workgroup: four waves, one lane per ray");

// INNER_X: d_vol's x axis is its contiguous one (the (1, D, H, W) tensor seen through RayBundleProjector); otherwise z is
template <typename VT, bool INNER_X>
__global__ __launch_bounds__(PBW_GROUP) void project_bundle_bwd_window_kernel(ProjBundleParams<VT> P) {
    __shared__ float box[PBW_BOX];
    __shared__ int red_i[6][4];
    __shared__ float red_f[2][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = bundle_ray();
    const VolView<VT> vol = P.vol;
    const GradView dv = P.dvol;

    RayGeom rg;
    rg.n = 0; rg.entry = rg.exit_ = rg.t0 = 0.0f; rg.vx = rg.vy = rg.vz = 0.0f;
    f3 o = make_f3(0.f, 0.f, 0.f);
    int m = 0;
    float gd = 0.0f;
    if (p < P.N) {
        o = load_f3(P.cam, p);
        load_ray(P.entry, P.exit_, P.rays, P.nsamp, p, rg);
        m = bundle_proj_samples(rg.n, P.S);
        gd = m > 0 ? finite_or_zero(P.grad_out[p] * bundle_proj_delta(rg)) : 0.0f;
        if (gd == 0.0f) m = 0;
    }
    // the group's depth range
    float tlo = m > 0 ? rg.t0 : __builtin_inff(), thi = m > 0 ? rg.exit_ : -__builtin_inff();
    tlo = wave_minf(tlo); thi = wave_maxf(thi);
    if (lane == 0) { red_f[0][wave] = tlo; red_f[1][wave] = thi; }
    __syncthreads();
    tlo = fminf(fminf(red_f[0][0], red_f[0][1]), fminf(red_f[0][2], red_f[0][3]));
    thi = fmaxf(fmaxf(red_f[1][0], red_f[1][1]), fmaxf(red_f[1][2], red_f[1][3]));
    if (!(tlo <= thi)) return;   // no live ray in the group (uniform)
    // sample index of t on this ray: s/(n-1) = (t - t0)/(exit - t0)
    const float s_per_t = m > 0 ? (float)(rg.n - 1) / (rg.exit_ - rg.t0) : 0.0f;

    constexpr int BIG = 0x3fffffff;
    int s_cur = 0;
    float tw0 = tlo, d = P.win_t0;
    for (;;) {
        const float tw1 = tw0 + d;
        const bool last = !(tw1 < thi) || !(tw1 > tw0);   // (a window below the ulp of t would not move on)
        int s_end = m;
        if (!last) {
            const float k = fminf(fmaxf((tw1 - rg.t0) * s_per_t, 0.0f), (float)m);
            s_end = max(s_cur, (int)ceilf(k));
        }
        // the cells of this lane's first and last sample in the window
        int b[6] = {BIG, BIG, BIG, -BIG, -BIG, -BIG};
        if (s_cur < s_end) {
            float px, py, pz;
            Cell c0, c1;
            sample_pos(rg, o.x, o.y, o.z, s_cur, px, py, pz);
            tri_cell(vol, px, py, pz, c0);
            sample_pos(rg, o.x, o.y, o.z, s_end - 1, px, py, pz);
            tri_cell(vol, px, py, pz, c1);
            b[0] = min(c0.x0, c1.x0); b[3] = max(c0.x1, c1.x1);
            b[1] = min(c0.y0, c1.y0); b[4] = max(c0.y1, c1.y1);
            b[2] = min(c0.z0, c1.z0); b[5] = max(c0.z1, c1.z1);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) { b[q] = wave_min(b[q]); b[q + 3] = wave_max(b[q + 3]); }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) red_i[q][wave] = b[q];
        }
        __syncthreads();
        const int bx0 = min(min(red_i[0][0], red_i[0][1]), min(red_i[0][2], red_i[0][3]));
        const int by0 = min(min(red_i[1][0], red_i[1][1]), min(red_i[1][2], red_i[1][3]));
        const int bz0 = min(min(red_i[2][0], red_i[2][1]), min(red_i[2][2], red_i[2][3]));
        const int bx1 = max(max(red_i[3][0], red_i[3][1]), max(red_i[3][2], red_i[3][3]));
        const int by1 = max(max(red_i[4][0], red_i[4][1]), max(red_i[4][2], red_i[4][3]));
        const int bz1 = max(max(red_i[5][0], red_i[5][1]), max(red_i[5][2], red_i[5][3]));
        __syncthreads();   // red_i is read by every lane before the next window writes it
        const bool any = bx0 <= bx1;
        const int nx = bx1 - bx0 + 1, ny = by1 - by0 + 1, nz = bz1 - bz0 + 1;   // (BIG: no overflow where no lane is active)
        const int64_t nvox = any ? (int64_t)nx * ny * nz : 0;
        if (nvox > PBW_BOX && d > P.win_tmin) { d *= 0.5f; continue; }   // a shallower window (no sample taken yet)

        if (nvox > PBW_BOX) {
            // an incoherent group: everything that is left, per tap (uniform: the group leaves together)
            for (int s = s_cur; s < m; ++s) {
                float px, py, pz;
                sample_pos(rg, o.x, o.y, o.z, s, px, py, pz);
                tri_scatter_global(vol, dv, px, py, pz, gd);
            }
            return;
        }
        if (nvox > 0) {
            const int lx = INNER_X ? 1 : nz * ny, ly = INNER_X ? nx : nz, lz = INNER_X ? nx * ny : 1;
            for (int k = threadIdx.x; k < (int)nvox; k += PBW_GROUP) box[k] = 0.0f;
            __syncthreads();
            for (int s = s_cur; s < s_end; ++s) {
                float px, py, pz;
                sample_pos(rg, o.x, o.y, o.z, s, px, py, pz);
                Cell c;
                tri_cell(vol, px, py, pz, c);
                const float gx = 1.0f - c.fx, gy = 1.0f - c.fy, gz = 1.0f - c.fz;
                const int xs[2] = {c.x0, c.x1}, ys[2] = {c.y0, c.y1}, zs[2] = {c.z0, c.z1};
                const float wx[2] = {gx, c.fx}, wy[2] = {gy, c.fy}, wz[2] = {gz, c.fz};
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int x = xs[q & 1], y = ys[(q >> 1) & 1], z = zs[q >> 2];
                    const float w = wx[q & 1] * wy[(q >> 1) & 1] * wz[q >> 2] * gd;
                    const unsigned ux = (unsigned)(x - bx0), uy = (unsigned)(y - by0), uz = (unsigned)(z - bz0);
                    if (ux < (unsigned)nx && uy < (unsigned)ny && uz < (unsigned)nz)
                        atomicAdd(box + (ux * lx + uy * ly + uz * lz), w);
                    else
                        unsafeAtomicAdd(dv.p + x * dv.sx + y * dv.sy + z * dv.sz, w);
                }
            }
            __syncthreads();
            for (int k = threadIdx.x; k < (int)nvox; k += PBW_GROUP) {
                const float v = box[k];
                if (v == 0.0f) continue;
                int x, y, z;
                if (INNER_X) { x = k % nx; y = (k / nx) % ny; z = k / (nx * ny); }
                else { z = k % nz; y = (k / nz) % ny; x = k / (nz * ny); }
                unsafeAtomicAdd(dv.p + (bx0 + x) * dv.sx + (by0 + y) * dv.sy + (bz0 + z) * dv.sz, v);
            }
            __syncthreads();   // the box is cleared by the next window
        }
        s_cur = s_end;
        tw0 = tw1;
        if (last) break;
    }
}

// d origin and d direction of one ray, both modes: project_cam_kernel's walk and its five sums with coef = g D for SUM and
// coef = g at the stored argmax for MAX (the same frozen branches),
//   sP = sum grad mu, sTP = sum t_s grad mu, s0 = sum (1 - f_s)(grad mu . d), s1 = sum f_s (grad mu . d), smu = sum mu,
// then march_bundle.hip's once-per-ray tail through the slab faces the forward picked. With A = (1 - u/n)(1 - 0.5/n) and
// E = g smu (1 - u/n) / n (SUM: D's own dependence on tmin and tmax; else 0):
//   k_min = coef s0 A - E,   k_max = coef (s0 (1 - A) + s1) + E,
//   d origin = coef sP  + k_min grad_o tmin + k_max grad_o tmax,   grad_o tmin = -e_a / d_a,
//   d dir    = coef sTP + k_min grad_d tmin + k_max grad_d tmax,   grad_d tmin = -(tmin / d_a) e_a;
// k_min = 0 where the t_near clamp was taken. d dir is the gradient w.r.t. the direction as a free 3-vector (D19). No reduction,
// no atomic: each lane stores its six floats.
template <typename VT, int MODE>
__global__ __launch_bounds__(256) void project_bundle_ray_grad_kernel(ProjBundleParams<VT> P) {
    const int p = bundle_ray();
    if (p >= P.N) return;
    f3 d_o = make_f3(0.f, 0.f, 0.f), d_d = make_f3(0.f, 0.f, 0.f);
    if (P.nsamp[p] > 1) {
        Ray<VT> ray;
        open_bundle_ray<false>(ray, p, P.vol, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
        const VolView<VT> &vol = ray.vol;
        const RayGeom &rg = ray.rg;
        const f3 lf = ray.cam, vd = ray.vd;
        const int m = bundle_proj_samples(rg.n, P.S);
        const float g = P.grad_out[p];
        f3 sP = make_f3(0.f, 0.f, 0.f), sTP = make_f3(0.f, 0.f, 0.f);
        float s0 = 0.f, s1 = 0.f, smu = 0.f, coef;
        int s = 0, s_stop = m;
        if (MODE == DR_PROJ_MAX) {
            s = P.arg_max[p];
            s_stop = (s >= 0 && s < m) ? s + 1 : s;
            coef = g;
        } else {
            coef = g * bundle_proj_delta(rg);
        }
        for (; s < s_stop; ++s) {
            float px, py, pz;
            sample_pos(ray, s, px, py, pz);
            f3 gI;
            smu += tri_sample_grad(vol, px, py, pz, gI);
            const float f = (float)s / (float)(rg.n - 1);
            const float t = mixf(rg.t0, rg.exit_, f);
            const float gv = dot3(gI, vd);
            sP = f3_add(sP, gI);
            sTP = f3_fma(t, gI, sTP);
            s0 = fmaf(1.0f - f, gv, s0);
            s1 = fmaf(f, gv, s1);
        }

        // once per ray: the faces the forward picked, the t_near clamp it took, the jitter draw behind A and E
        const SlabFaces sf = slab_faces(lf, vd);
        const bool clamped = P.t_near > -INFINITY && sf.tmin < P.t_near;
        const float nf = (float)rg.n;
        const float u = P.jitter_seed != 0u ? jitter_u(P.jitter_seed, P.ray_base, (uint32_t)p) : 0.0f;
        const float Acoef = (1.0f - u / nf) * (1.0f - 0.5f / nf);
        const float E = (MODE == DR_PROJ_SUM && m > 0) ? ((g * smu) / nf) * (1.0f - u / nf) : 0.0f;
        const float k_min = clamped ? 0.0f : coef * (s0 * Acoef) - E, k_max = coef * fmaf(s0, 1.0f - Acoef, s1) + E;
        const f3 emin = make_f3(sf.amin == 0 ? 1.0f : 0.0f, sf.amin == 1 ? 1.0f : 0.0f, sf.amin == 2 ? 1.0f : 0.0f);
        const f3 emax = make_f3(sf.amax == 0 ? 1.0f : 0.0f, sf.amax == 1 ? 1.0f : 0.0f, sf.amax == 2 ? 1.0f : 0.0f);
        const float cmin = -k_min * sf.ivmin, cmax = -k_max * sf.ivmax;
        d_o = f3_fma(cmax, emax, f3_fma(cmin, emin, f3_scale(coef, sP)));
        d_d = f3_fma(cmax * sf.tmax, emax, f3_fma(cmin * sf.tmin, emin, f3_scale(coef, sTP)));
        // D5: a NaN ray (NaN upstream gradient) contributes nothing, infinities are clamped
        d_o = make_f3(finite_or_zero(d_o.x), finite_or_zero(d_o.y), finite_or_zero(d_o.z));
        d_d = make_f3(finite_or_zero(d_d.x), finite_or_zero(d_d.y), finite_or_zero(d_d.z));
    }
    const size_t q = 3 * (size_t)p;
    P.d_origins[q] = d_o.x; P.d_origins[q + 1] = d_o.y; P.d_origins[q + 2] = d_o.z;
    P.d_dirs[q] = d_d.x; P.d_dirs[q + 1] = d_d.y; P.d_dirs[q + 2] = d_d.z;
}

template <typename VT>
static ProjBundleParams<VT> proj_bundle_params(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q) {
    ProjBundleParams<VT> P{make_ray_params<VT>(a)};
    P.cam = b.origins;
    P.N = b.N; P.arg_max = q.arg_max;
    // window depths in world units: a voxel of the finest axis is 2 / (V - 1) of the [-1, 1] box
    const float vox = 2.0f / (float)(max(a.VX, max(a.VY, a.VZ)) - 1);
    P.win_t0 = PBW_WIN_VOX * vox; P.win_tmin = PBW_MIN_VOX * vox;
    P.t_near = b.t_near; P.jitter_seed = b.jitter_seed; P.ray_base = b.ray_base;
    P.d_origins = b.d_origins; P.d_dirs = b.d_dirs;
    return P;
}

template <typename VT>
static int proj_bundle_fwd_dispatch(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream) {
    return launch_bundle(q.mode == DR_PROJ_SUM ? project_bundle_fwd_kernel<VT, DR_PROJ_SUM> : project_bundle_fwd_kernel<VT, DR_PROJ_MAX>,
                         b.N, 0, stream, proj_bundle_params<VT>(a, b, q));
}

template <typename VT>
static int proj_bundle_bwd_dispatch(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream) {
    const ProjBundleParams<VT> P = proj_bundle_params<VT>(a, b, q);
    if (q.mode == DR_PROJ_MAX) return launch_bundle(project_bundle_bwd_plain_kernel<VT, DR_PROJ_MAX>, b.N, 0, stream, P);
    if (q.variant == DR_VARIANT_BASELINE) return launch_bundle(project_bundle_bwd_plain_kernel<VT, DR_PROJ_SUM>, b.N, 0, stream, P);
    const bool inner_x = (a.dsx < 0 ? -a.dsx : a.dsx) <= (a.dsz < 0 ? -a.dsz : a.dsz);
    return launch_bundle(inner_x ? project_bundle_bwd_window_kernel<VT, true> : project_bundle_bwd_window_kernel<VT, false>, b.N, 0,
                         stream, P);
}

template <typename VT>
static int proj_bundle_ray_grad_dispatch(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream) {
    return launch_bundle(q.mode == DR_PROJ_SUM ? project_bundle_ray_grad_kernel<VT, DR_PROJ_SUM>
                                               : project_bundle_ray_grad_kernel<VT, DR_PROJ_MAX>,
                         b.N, 0, stream, proj_bundle_params<VT>(a, b, q));
}

int launch_project_bundle_fwd(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? proj_bundle_fwd_dispatch<__half>(a, b, q, stream) : proj_bundle_fwd_dispatch<float>(a, b, q, stream);
}
int launch_project_bundle_bwd(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? proj_bundle_bwd_dispatch<__half>(a, b, q, stream) : proj_bundle_bwd_dispatch<float>(a, b, q, stream);
}
int launch_project_bundle_ray_grad(const MarchArgs &a, const BundleArgs &b, const ProjArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? proj_bundle_ray_grad_dispatch<__half>(a, b, q, stream)
                                 : proj_bundle_ray_grad_dispatch<float>(a, b, q, stream);
}

}  // namespace dr
