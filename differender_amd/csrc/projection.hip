// projection.hip -- X-ray line-integral (DR_PROJ_SUM) and maximum-intensity (DR_PROJ_MAX) projections and their gradients
// w.r.t. the volume and the camera position, for gfx950.
//
// The samples are those of the march (dr_device.h's sample_pos on the ray buffers of ray_setup.hip): s < m = min(n, S),
// pos_s = look_from + mix(t0, exit, s/(n-1)) vd, one trilinear tap each, no table, no shading. A ray with n <= 1 gives 0.
//   SUM: out = D sum_s mu(pos_s), D = (exit - entry) / n, the sum sequential in f32 and multiplied by D once;
//   MAX: out = max_s mu(pos_s), the first maximum by a strict > update; its index goes to arg_max (-1: no sample).
// The line integral is linear in the volume: its backward is a back-projection of g D onto the 8 trilinear weights of every
// sample. The plain backward does this with global float atomics per tap (one lane per ray); the windowed backward collects a
// pixel tile's taps of one depth window in LDS and adds the box to d_vol row by row (below).
#include "dr_camera.h"
#include "dr_tile.h"
#include "dr_wave.h"

namespace dr {

template <typename VT>
struct ProjParams : RayParams<VT> {
    int32_t *arg_max;   // MAX: the forward writes it, the backwards read it
    CamFields cf;       // camera backward
};

// samples of a ray (n <= 1: none, as H6)
__device__ __forceinline__ int proj_samples(int n, int S) { return n > 1 ? min(n, S) : 0; }
__device__ __forceinline__ float proj_delta(const RayGeom &rg) { return (rg.exit_ - rg.entry) / (float)rg.n; }

// Forward, both modes: one lane per ray, a wave per 8x8 pixel tile (march_baseline.hip's shape).
template <typename VT, int MODE>
__global__ __launch_bounds__(256) void project_fwd_kernel(ProjParams<VT> P) {
    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const int view = blockIdx.y;
    const size_t p = ray_index(P.W, P.H, view, i, j);
    Ray<VT> ray;
    open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
    const VolView<VT> &vol = ray.vol;
    const RayGeom &rg = ray.rg;
    const int m = proj_samples(rg.n, P.S);
    if (MODE == DR_PROJ_SUM) {
        float acc = 0.0f;
        for (int s = 0; s < m; ++s) {
            float px, py, pz;
            sample_pos(ray, s, px, py, pz);
            acc += tri_sample(vol, px, py, pz);
        }
        P.out[p] = m > 0 ? proj_delta(rg) * acc : 0.0f;
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

// Volume backward, one lane per ray with global float atomics per tap: SUM (every sample, weight g D) -- the yardstick of the
// windowed kernel and DR_VARIANT_BASELINE -- and MAX (the one stored argmax sample, weight g). (Its prologue is its own: through
// open_ray the MAX kernel's scalar loads merge differently.)
template <typename VT, int MODE>
__global__ __launch_bounds__(256) void project_bwd_plain_kernel(ProjParams<VT> P) {
    int i, j;
    if (!tile_pixel(P.W, P.H, i, j)) return;
    const int view = blockIdx.y;
    const size_t p = ((size_t)view * P.W + i) * P.H + j;
    VolView<VT> vol = P.vol;
    vol.p += view * P.vol_vs;
    GradView dv = P.dvol;
    dv.p += view * P.dvol_vs;
    const float cx = P.cam[3 * view], cy = P.cam[3 * view + 1], cz = P.cam[3 * view + 2];
    RayGeom rg;
    load_ray(P.entry, P.exit_, P.rays, P.nsamp, p, rg);
    const int m = proj_samples(rg.n, P.S);
    if (MODE == DR_PROJ_SUM) {
        const float gd = m > 0 ? finite_or_zero(P.grad_out[p] * proj_delta(rg)) : 0.0f;
        if (gd == 0.0f) return;
        for (int s = 0; s < m; ++s) {
            float px, py, pz;
            sample_pos(rg, cx, cy, cz, s, px, py, pz);
            tri_scatter_global(vol, dv, px, py, pz, gd);
        }
    } else {
        const int s = P.arg_max[p];
        const float g = finite_or_zero(P.grad_out[p]);
        if (s < 0 || s >= m || g == 0.0f) return;
        float px, py, pz;
        sample_pos(rg, cx, cy, cz, s, px, py, pz);
        tri_scatter_global(vol, dv, px, py, pz, g);
    }
}

// Windowed SUM backward. A 256-thread workgroup owns a 16x16 pixel tile (lane = pixel) and walks the tile's rays front to back
// through depth windows of t. Per window every lane takes its samples with t_s below the window's far end; the workgroup bounds
// the cells they touch by the cells of each lane's first and last sample in the window (a cell index is monotone along a ray, up
// to the last-place roundings of mix(): a tap that lands outside the box goes to global memory, as in the fallback; a margin of
// one cell instead made the kernel 1.3x slower: profiles/proj_kernel_stats.txt), adds g D w_tap into that box in LDS
// (ds_add_f32) and then adds
// the box to d_vol with global float atomics in the order of d_vol's contiguous axis, so that a wave-instruction covers row
// segments, not 64 scattered rows. A box above the LDS budget halves the window (down to PW_MIN_VOX voxels deep); a window that
// still does not fit (near cameras, wide fields of view, coarse images) goes to global atomics per tap, as the plain kernel.
constexpr int PW_TILE = 16;
constexpr int PW_BOX = 7680;        // LDS floats of the box: 30 KiB, five workgroups (20 waves) per CU by LDS
constexpr float PW_WIN_VOX = 16.0f;  // first window depth, in voxels of the finest axis
constexpr float PW_MIN_VOX = 2.0f;   // shallowest window before the global fallback

// INNER_X: d_vol's x axis is its contiguous one (the (1, D, H, W) tensor seen through Projector); otherwise z is (field order)
template <typename VT, bool INNER_X>
__global__ __launch_bounds__(256) void project_bwd_window_kernel(ProjParams<VT> P, float win_t0, float win_tmin) {
    __shared__ float box[PW_BOX];
    __shared__ int red_i[6][4];
    __shared__ float red_f[2][4];
    const int view = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles_j = (P.H + PW_TILE - 1) / PW_TILE;
    const int i = (blockIdx.x / tiles_j) * PW_TILE + (int)(threadIdx.x >> 4);
    const int j = (blockIdx.x % tiles_j) * PW_TILE + (int)(threadIdx.x & 15);
    VolView<VT> vol = P.vol;
    vol.p += view * P.vol_vs;
    GradView dv = P.dvol;
    dv.p += view * P.dvol_vs;
    const float cx = P.cam[3 * view], cy = P.cam[3 * view + 1], cz = P.cam[3 * view + 2];

    RayGeom rg;
    rg.n = 0; rg.entry = rg.exit_ = rg.t0 = 0.0f; rg.vx = rg.vy = rg.vz = 0.0f;
    int m = 0;
    float gd = 0.0f;
    if (i < P.W && j < P.H) {
        const size_t p = ((size_t)view * P.W + i) * P.H + j;
        load_ray(P.entry, P.exit_, P.rays, P.nsamp, p, rg);
        m = proj_samples(rg.n, P.S);
        gd = m > 0 ? finite_or_zero(P.grad_out[p] * proj_delta(rg)) : 0.0f;
        if (gd == 0.0f) m = 0;
    }
    // the tile's depth range
    float tlo = m > 0 ? rg.t0 : __builtin_inff(), thi = m > 0 ? rg.exit_ : -__builtin_inff();
    tlo = wave_minf(tlo); thi = wave_maxf(thi);
    if (lane == 0) { red_f[0][wave] = tlo; red_f[1][wave] = thi; }
    __syncthreads();
    tlo = fminf(fminf(red_f[0][0], red_f[0][1]), fminf(red_f[0][2], red_f[0][3]));
    thi = fmaxf(fmaxf(red_f[1][0], red_f[1][1]), fmaxf(red_f[1][2], red_f[1][3]));
    if (!(tlo <= thi)) return;   // no live ray in the tile (uniform)
    // sample index of t on this ray: s/(n-1) = (t - t0)/(exit - t0)
    const float s_per_t = m > 0 ? (float)(rg.n - 1) / (rg.exit_ - rg.t0) : 0.0f;

    constexpr int BIG = 0x7fffffff;
    int s_cur = 0;
    float tw0 = tlo, d = win_t0;
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
            sample_pos(rg, cx, cy, cz, s_cur, px, py, pz);
            tri_cell(vol, px, py, pz, c0);
            sample_pos(rg, cx, cy, cz, s_end - 1, px, py, pz);
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
        const int nx = bx1 - bx0 + 1, ny = by1 - by0 + 1, nz = bz1 - bz0 + 1;
        const int64_t nvox = any ? (int64_t)nx * ny * nz : 0;
        if (nvox > PW_BOX && d > win_tmin) { d *= 0.5f; continue; }   // a shallower window (no sample taken yet)

        if (nvox > 0 && nvox <= PW_BOX) {
            const int lx = INNER_X ? 1 : nz * ny, ly = INNER_X ? nx : nz, lz = INNER_X ? nx * ny : 1;
            for (int k = threadIdx.x; k < (int)nvox; k += 256) box[k] = 0.0f;
            __syncthreads();
            for (int s = s_cur; s < s_end; ++s) {
                float px, py, pz;
                sample_pos(rg, cx, cy, cz, s, px, py, pz);
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
            for (int k = threadIdx.x; k < (int)nvox; k += 256) {
                const float v = box[k];
                if (v == 0.0f) continue;
                int x, y, z;
                if (INNER_X) { x = k % nx; y = (k / nx) % ny; z = k / (nx * ny); }
                else { z = k % nz; y = (k / nz) % ny; x = k / (nz * ny); }
                unsafeAtomicAdd(dv.p + (bx0 + x) * dv.sx + (by0 + y) * dv.sy + (bz0 + z) * dv.sz, v);
            }
            __syncthreads();   // the box is cleared by the next window
        } else if (nvox > 0) {
            for (int s = s_cur; s < s_end; ++s) {
                float px, py, pz;
                sample_pos(rg, cx, cy, cz, s, px, py, pz);
                tri_scatter_global(vol, dv, px, py, pz, gd);
            }
        }
        s_cur = s_end;
        tw0 = tw1;
        if (last) break;
    }
}

// Camera backward, both modes (camera_grad.hip's structure and its D8 chain, without lighting): per sample
//   P_s = c dmu/dpos_s  (c = g D for SUM, g for the MAX sample), and per ray
//   d look_from = sum P_s + J_vd^T sum t_s P_s + sum (1-f_s)(P_s.vd) grad t0 + sum f_s (P_s.vd) grad tmax
//                 [+ g (sum mu_s) (grad tmax - grad entry) / n   for SUM: D's own dependence on the camera],
//   grad t0 = A grad tmin + (1-A) grad tmax, A = (1 - u/n)(1 - 0.5/n), grad entry = grad tmin + (u/n)(grad tmax - grad tmin).
// Sums in f32 per ray, f64 per workgroup (LDS), one f64 atomic per component per workgroup.
// POSE: the ten pose gradients of the free camera instead (dr_camera.h: pose_ray_grad, pose_reduce) -- the same sums, with the
// weights of grad tmin and grad tmax collected: coef s0 A - E and coef (s0 (1 - A) + s1) + E, E = g (sum mu_s) (1 - u/n) / n.
template <typename VT, int MODE, bool POSE>
__global__ __launch_bounds__(256) void project_cam_kernel(ProjParams<VT> P) {
    __shared__ double red[3][256];
    const int view = blockIdx.y;
    f3 dcam = make_f3(0.f, 0.f, 0.f);
    PoseGrad dpose = pose_zero();
    int i, j;
    const bool in_img = tile_pixel(P.W, P.H, i, j);
    const size_t p = ray_index(P.W, P.H, view, i, j);
    if (in_img && P.nsamp[p] > 1) {
        Ray<VT> ray;
        open_ray<false>(ray, view, p, P.vol, P.vol_vs, P.cam, P.entry, P.exit_, P.rays, P.nsamp);
        const VolView<VT> &vol = ray.vol;
        const RayGeom &rg = ray.rg;
        const f3 lf = ray.cam, vd = ray.vd;
        const int m = proj_samples(rg.n, P.S);
        const float g = P.grad_out[p];
        f3 sP = make_f3(0.f, 0.f, 0.f), sTP = make_f3(0.f, 0.f, 0.f);
        float s0 = 0.f, s1 = 0.f, smu = 0.f, coef;
        int s = 0, s_stop = m;
        if (MODE == DR_PROJ_MAX) {
            s = P.arg_max[p];
            s_stop = (s >= 0 && s < m) ? s + 1 : s;
            coef = g;
        } else {
            coef = g * proj_delta(rg);
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
        if (POSE) {
            // once per ray: the ten pose gradients from the same sums (dr_camera.h; a projection is never a band), then D5
            const PoseRay q = pose_ray(P.cf.pose, P.cf.fov_v, view, P.cf.near_d, P.cf.aspect, P.cf.near_w, P.cf.near_h, i, P.W, j,
                                       P.H, rg.n, P.cf.jitter_seed, P.cf.view_base + (uint32_t)view);
            const float nf = (float)rg.n;
            const float E = (MODE == DR_PROJ_SUM && m > 0) ? ((g * smu) / nf) * (1.0f - q.jit / nf) : 0.0f;
            dpose = pose_finite(pose_ray_grad(lf, q, vd, P.cf.near_, f3_scale(coef, sP), f3_scale(coef, sTP),
                                              coef * (s0 * q.A) - E, coef * fmaf(s0, 1.0f - q.A, s1) + E));
        } else {
            // once per ray: J_vd, the rows of the slab faces the forward picked and the jitter draw (a projection is never a band)
            M3 J;
            f3 g_tmin, g_tmax, g_t0;
            float u;
            camera_ray_tail(lf, vd, i, P.W, j, P.H, P.cf.near_, P.cf.near_w, P.cf.near_h, rg.n, P.cf.jitter_seed,
                            P.cf.view_base + (uint32_t)view, J, g_tmin, g_tmax, g_t0, u);
            const float nf = (float)rg.n;
            f3 dpos = f3_add(sP, mul_t(J, sTP));
            dpos = f3_fma(s0, g_t0, dpos);
            dpos = f3_fma(s1, g_tmax, dpos);
            dcam = f3_scale(coef, dpos);
            if (MODE == DR_PROJ_SUM && m > 0) {
                const f3 g_entry = f3_fma(u / nf, f3_add(g_tmax, f3_scale(-1.0f, g_tmin)), g_tmin);
                dcam = f3_fma((g * smu) / nf, f3_add(g_tmax, f3_scale(-1.0f, g_entry)), dcam);
            }
            // D5: a NaN ray contributes nothing, infinities are clamped
            dcam = make_f3(finite_or_zero(dcam.x), finite_or_zero(dcam.y), finite_or_zero(dcam.z));
        }
    }
    if (POSE) pose_reduce(dpose, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
    else camera_reduce(dcam, in_img, p, view, P.cf.d_cam_ray, P.cf.d_cam, red);
}

template <typename VT>
static ProjParams<VT> proj_params(const MarchArgs &a, const ProjArgs &q) {
    ProjParams<VT> P{make_ray_params<VT>(a)};
    P.arg_max = q.arg_max;
    P.cf = fill_cam_fields(a, q.jitter_seed, q.view_base, q.d_cam, q.d_cam_ray);   // (fill_proj: img_W = W)
    return P;
}

template <typename VT>
static int fwd_dispatch(const MarchArgs &a, const ProjArgs &q, hipStream_t stream) {
    const ProjParams<VT> P = proj_params<VT>(a, q);
    return launch_tiles(q.mode == DR_PROJ_SUM ? project_fwd_kernel<VT, DR_PROJ_SUM> : project_fwd_kernel<VT, DR_PROJ_MAX>, a, 0,
                        stream, P);
}

template <typename VT>
static int bwd_dispatch(const MarchArgs &a, const ProjArgs &q, hipStream_t stream) {
    const ProjParams<VT> P = proj_params<VT>(a, q);
    if (q.mode == DR_PROJ_MAX) return launch_tiles(project_bwd_plain_kernel<VT, DR_PROJ_MAX>, a, 0, stream, P);
    if (q.variant == DR_VARIANT_BASELINE) return launch_tiles(project_bwd_plain_kernel<VT, DR_PROJ_SUM>, a, 0, stream, P);
    // window depths in world units: a voxel of the finest axis is 2 / (V - 1) of the [-1, 1] box
    const float vox = 2.0f / (float)(max(a.VX, max(a.VY, a.VZ)) - 1);
    const bool inner_x = (a.dsx < 0 ? -a.dsx : a.dsx) <= (a.dsz < 0 ? -a.dsz : a.dsz);
    const int tiles = ((a.W + PW_TILE - 1) / PW_TILE) * ((a.H + PW_TILE - 1) / PW_TILE);
    void (*kernel)(ProjParams<VT>, float, float) = inner_x ? project_bwd_window_kernel<VT, true> : project_bwd_window_kernel<VT, false>;
    hipLaunchKernelGGL(kernel, dim3(tiles, a.n_views), dim3(256), 0, stream, P, PW_WIN_VOX * vox, PW_MIN_VOX * vox);
    return (int)hipGetLastError();
}

template <typename VT>
static int cam_dispatch(const MarchArgs &a, const ProjArgs &q, hipStream_t stream) {
    const ProjParams<VT> P = proj_params<VT>(a, q);
    if (a.pose)
        return launch_tiles(q.mode == DR_PROJ_SUM ? project_cam_kernel<VT, DR_PROJ_SUM, true> : project_cam_kernel<VT, DR_PROJ_MAX, true>,
                            a, 0, stream, P);
    return launch_tiles(q.mode == DR_PROJ_SUM ? project_cam_kernel<VT, DR_PROJ_SUM, false> : project_cam_kernel<VT, DR_PROJ_MAX, false>,
                        a, 0, stream, P);
}

int launch_project_fwd(const MarchArgs &a, const ProjArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? fwd_dispatch<__half>(a, q, stream) : fwd_dispatch<float>(a, q, stream);
}
int launch_project_bwd(const MarchArgs &a, const ProjArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? bwd_dispatch<__half>(a, q, stream) : bwd_dispatch<float>(a, q, stream);
}
int launch_project_bwd_cam(const MarchArgs &a, const ProjArgs &q, hipStream_t stream) {
    return a.vol_dtype == DR_F16 ? cam_dispatch<__half>(a, q, stream) : cam_dispatch<float>(a, q, stream);
}

}  // namespace dr
