// dr_camera.h -- the chain rule of the camera position look_from through ray setup, shared by the camera
// gradients of the march (camera_grad.hip) and of the projections (projection.hip): the Jacobian of the ray direction, the
// gradients of the slab distances, and the rows of the faces a ray's entry and exit picked (VR.py:28-53, 127-151).
#pragma once
#include "dr_device.h"

namespace dr {

struct M3 { f3 r0, r1, r2; };  // rows
__device__ __forceinline__ f3 f3_add(f3 a, f3 b) { return make_f3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 f3_scale(float s, f3 a) { return make_f3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ f3 f3_fma(float s, f3 a, f3 b) { return make_f3(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z)); }
__device__ __forceinline__ f3 cross_f3(f3 a, f3 b) {
    return make_f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ f3 mul_t(const M3 &m, f3 g) {   // m^T g
    return make_f3(m.r0.x * g.x + m.r1.x * g.y + m.r2.x * g.z, m.r0.y * g.x + m.r1.y * g.y + m.r2.y * g.z,
                   m.r0.z * g.x + m.r1.z * g.y + m.r2.z * g.z);
}
__device__ __forceinline__ f3 col(const M3 &m, int k) {
    return k == 0 ? make_f3(m.r0.x, m.r1.x, m.r2.x) : (k == 1 ? make_f3(m.r0.y, m.r1.y, m.r2.y) : make_f3(m.r0.z, m.r1.z, m.r2.z));
}
__device__ __forceinline__ M3 from_cols(f3 c0, f3 c1, f3 c2) {
    M3 m;
    m.r0 = make_f3(c0.x, c1.x, c2.x); m.r1 = make_f3(c0.y, c1.y, c2.y); m.r2 = make_f3(c0.z, c1.z, c2.z);
    return m;
}
// Jacobian of normalize(x) applied to the columns of dx: (I - y y^T) dx / |x|
__device__ __forceinline__ M3 d_normalize(f3 y, float inv_len, const M3 &dx) {
    f3 c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f3 d = col(dx, k);
        c[k] = f3_scale(inv_len, f3_fma(-dot3(y, d), y, d));
    }
    return from_cols(c[0], c[1], c[2]);
}
__device__ __forceinline__ float inv_norm3(f3 a) { return 1.0f / sqrtf(dot3(a, a)); }

// d vd / d look_from of VR.py:127-151 for the pixel with near-plane offsets (uw, vh): view_dir = normalize(-lf),
// right = normalize(view_dir x e_y), up = normalize(right x view_dir), vd = normalize(near view_dir + uw right + vh up).
// A camera on the y axis has right = 0 (degenerate in the forward already).
__device__ __forceinline__ M3 ray_dir_jacobian(f3 lf, float near_, float uw, float vh) {
    const f3 a = make_f3(-lf.x, -lf.y, -lf.z);
    const float ia = inv_norm3(a);
    const f3 vdir = f3_scale(ia, a);
    M3 I3; I3.r0 = make_f3(-1.f, 0.f, 0.f); I3.r1 = make_f3(0.f, -1.f, 0.f); I3.r2 = make_f3(0.f, 0.f, -1.f);   // d(-lf)/dlf
    const M3 Jv = d_normalize(vdir, ia, I3);
    const f3 c = cross_f3(vdir, make_f3(0.f, 1.f, 0.f));                 // (-vdir.z, 0, vdir.x)
    const float ic = inv_norm3(c);
    const f3 right = f3_scale(ic, c);
    M3 Jc; Jc.r0 = f3_scale(-1.f, Jv.r2); Jc.r1 = make_f3(0.f, 0.f, 0.f); Jc.r2 = Jv.r0;
    const M3 Jr = d_normalize(right, ic, Jc);
    const f3 d = cross_f3(right, vdir);
    const float id = inv_norm3(d);
    const f3 up = f3_scale(id, d);
    f3 dc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dc[k] = f3_add(cross_f3(col(Jr, k), vdir), cross_f3(right, col(Jv, k)));
    const M3 Ju = d_normalize(up, id, from_cols(dc[0], dc[1], dc[2]));
    const f3 w = f3_add(f3_add(f3_scale(near_, vdir), f3_scale(uw, right)), f3_scale(vh, up));
    const float iw = inv_norm3(w);
    f3 wc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) wc[k] = f3_add(f3_add(f3_scale(near_, col(Jv, k)), f3_scale(uw, col(Jr, k))), f3_scale(vh, col(Ju, k)));
    return d_normalize(f3_scale(iw, w), iw, from_cols(wc[0], wc[1], wc[2]));
}

// gradient of one slab distance t = (c - lf_a) / vd_a w.r.t. look_from (through lf_a and vd_a)
__device__ __forceinline__ f3 slab_grad(int axis, float t, float inv_vda, const M3 &J) {
    // (a weighted sum of the rows, not a selected one: a selected struct member is an indexed private array, i.e. scratch)
    const float w0 = axis == 0 ? 1.0f : 0.0f, w1 = axis == 1 ? 1.0f : 0.0f, w2 = axis == 2 ? 1.0f : 0.0f;
    const f3 row = f3_add(f3_add(f3_scale(w0, J.r0), f3_scale(w1, J.r1)), f3_scale(w2, J.r2));
    return f3_fma(-inv_vda, make_f3(w0, w1, w2), f3_scale(-t * inv_vda, row));
}

// The slab distances of the ray from lf along vd (ray_setup.hip's arithmetic) and the gradients of tmin and tmax through the
// faces they picked (frozen), given J = d vd / d look_from.
__device__ __forceinline__ void slab_rows(f3 lf, f3 vd, const M3 &J, f3 &g_tmin, f3 &g_tmax) {
    const float fx = 1.0f / vd.x, fy = 1.0f / vd.y, fz = 1.0f / vd.z;
    const float t1 = (-1.0f - lf.x) * fx, t2 = (1.0f - lf.x) * fx;
    const float t3 = (-1.0f - lf.y) * fy, t4 = (1.0f - lf.y) * fy;
    const float t5 = (-1.0f - lf.z) * fz, t6 = (1.0f - lf.z) * fz;
    const float lo_x = fminf(t1, t2), lo_y = fminf(t3, t4), lo_z = fminf(t5, t6);
    const float hi_x = fmaxf(t1, t2), hi_y = fmaxf(t3, t4), hi_z = fmaxf(t5, t6);
    const float tmin = fmaxf(fmaxf(lo_x, lo_y), lo_z), tmax = fminf(fminf(hi_x, hi_y), hi_z);
    const int amin = (tmin == lo_x) ? 0 : ((tmin == lo_y) ? 1 : 2);
    const int amax = (tmax == hi_x) ? 0 : ((tmax == hi_y) ? 1 : 2);
    const float ivmin = amin == 0 ? fx : (amin == 1 ? fy : fz), ivmax = amax == 0 ? fx : (amax == 1 ? fy : fz);
    g_tmin = slab_grad(amin, tmin, ivmin, J);
    g_tmax = slab_grad(amax, tmax, ivmax, J);
}

// The near-plane extents of VR.py:146-147 as ray_setup.hip forms them: doubles, rounded once (host side of the two camera
// backwards; img_W: the rows of the whole image, of which a band call renders W).
inline void near_plane_extents(double fov_rad, double near_plane, int img_W, int H, float &near_, float &near_w, float &near_h) {
    const double h = 2.0 * tan(fov_rad) * near_plane;
    const double w = h * ((double)img_W / (double)H);
    near_ = (float)near_plane; near_w = (float)w; near_h = (float)h;
}

// Once per ray: J = d vd / d look_from and the rows of the slab faces the forward picked (VR.py:28-53, same arithmetic as
// ray_setup.hip), the jitter draw u, and grad t0 = A grad tmin + (1-A) grad tmax, A = (1 - u/n)(1 - 0.5/n). row: the pixel's
// row within the whole image of img_W rows (a band adds its row0), j its column of H.
__device__ __forceinline__ void camera_ray_tail(f3 lf, f3 vd, int row, int img_W, int j, int H, float near_, float near_w,
                                                float near_h, int n, uint32_t jitter_seed, uint32_t view, M3 &J, f3 &g_tmin,
                                                f3 &g_tmax, f3 &g_t0, float &u) {
    const float x = ((float)row + 0.5f) / (float)img_W;
    const float y = ((float)j + 0.5f) / (float)H;
    J = ray_dir_jacobian(lf, near_, (x - 0.5f) * near_w, (y - 0.5f) * near_h);
    slab_rows(lf, vd, J, g_tmin, g_tmax);
    const float nf = (float)n;
    u = jitter_seed != 0u ? jitter_u(jitter_seed, view, (uint32_t)(row * H + j)) : 0.0f;
    const float Acoef = (1.0f - u / nf) * (1.0f - 0.5f / nf);
    g_t0 = f3_fma(Acoef, g_tmin, f3_scale(1.0f - Acoef, g_tmax));
}

// The end of both camera backwards (256 lanes, every lane arrives): the optional per-ray store, then the workgroup's sum in
// double (LDS tree) and ONE f64 atomic per component into d_cam[view][3]. p: the ray's index, read only where in_img.
__device__ __forceinline__ void camera_reduce(f3 dcam, bool in_img, size_t p, int view, float *d_cam_ray, double *d_cam,
                                              double (&red)[3][256]) {
    if (in_img && d_cam_ray) {
        d_cam_ray[3 * p] = dcam.x; d_cam_ray[3 * p + 1] = dcam.y; d_cam_ray[3 * p + 2] = dcam.z;
    }
    red[0][threadIdx.x] = (double)dcam.x; red[1][threadIdx.x] = (double)dcam.y; red[2][threadIdx.x] = (double)dcam.z;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
            red[2][threadIdx.x] += red[2][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3 && red[threadIdx.x][0] != 0.0) atomicAdd(d_cam + 3 * view + threadIdx.x, red[threadIdx.x][0]);
}

}  // namespace dr
