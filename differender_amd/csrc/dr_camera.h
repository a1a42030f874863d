// dr_camera.h -- the chain rule of the camera position look_from through ray setup, shared by the camera
// gradients of the march (camera_grad.hip) and of the projections (projection.hip): the Jacobian of the ray direction, the
// gradients of the slab distances, and the rows of the faces a ray's entry and exit picked (VR.py:28-53, 127-151); the
// once-per-ray tails and the reductions (march_rgba.hip's camera gradient too), and the kernel parameters every camera backward
// adds to its march's, with their one builder.
#pragma once
#include "dr_device.h"
#include "dr_kernels.h"

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

// The slab distances of the ray from lf along vd (ray_setup.hip's arithmetic) and the faces fmaxf / fminf picked for tmin and
// tmax (frozen in both camera backwards): their axes and 1 / vd on them.
struct SlabFaces { float tmin, tmax, ivmin, ivmax; int amin, amax; };
__device__ __forceinline__ SlabFaces slab_faces(f3 lf, f3 vd) {
    const float fx = 1.0f / vd.x, fy = 1.0f / vd.y, fz = 1.0f / vd.z;
    const float t1 = (-1.0f - lf.x) * fx, t2 = (1.0f - lf.x) * fx;
    const float t3 = (-1.0f - lf.y) * fy, t4 = (1.0f - lf.y) * fy;
    const float t5 = (-1.0f - lf.z) * fz, t6 = (1.0f - lf.z) * fz;
    const float lo_x = fminf(t1, t2), lo_y = fminf(t3, t4), lo_z = fminf(t5, t6);
    const float hi_x = fmaxf(t1, t2), hi_y = fmaxf(t3, t4), hi_z = fmaxf(t5, t6);
    SlabFaces s;
    s.tmin = fmaxf(fmaxf(lo_x, lo_y), lo_z); s.tmax = fminf(fminf(hi_x, hi_y), hi_z);
    s.amin = (s.tmin == lo_x) ? 0 : ((s.tmin == lo_y) ? 1 : 2);
    s.amax = (s.tmax == hi_x) ? 0 : ((s.tmax == hi_y) ? 1 : 2);
    s.ivmin = s.amin == 0 ? fx : (s.amin == 1 ? fy : fz); s.ivmax = s.amax == 0 ? fx : (s.amax == 1 ? fy : fz);
    return s;
}

// The gradients of tmin and tmax through the faces they picked, given J = d vd / d look_from.
__device__ __forceinline__ void slab_rows(f3 lf, f3 vd, const M3 &J, f3 &g_tmin, f3 &g_tmax) {
    const SlabFaces s = slab_faces(lf, vd);
    g_tmin = slab_grad(s.amin, s.tmin, s.ivmin, J);
    g_tmax = slab_grad(s.amax, s.tmax, s.ivmax, J);
}

// The near-plane extents of VR.py:146-147 as ray_setup.hip forms them: doubles, rounded once (host side of the two camera
// backwards; img_W: the rows of the whole image, of which a band call renders W).
inline void near_plane_extents(double fov_rad, double near_plane, int img_W, int H, float &near_, float &near_w, float &near_h) {
    const double h = 2.0 * tan(fov_rad) * near_plane;
    const double w = h * ((double)img_W / (double)H);
    near_ = (float)near_plane; near_w = (float)w; near_h = (float)h;
}

// What a camera backward reads beside its march's parameters: the near plane as ray_setup.hip formed it, the jitter seed, the
// outputs, and the free camera (a kernel's parameter struct embeds this after its own fields).
struct CamFields {
    float near_, near_w, near_h;
    uint32_t jitter_seed, view_base;
    double *d_cam; float *d_cam_ray;
    const float *pose, *fov_v;   // POSE: [views][9] look_from, look_at, up; [views] fov in radians, nullable
    double near_d, aspect;       // ... the near plane and img_W / H as doubles, for a view's own extents
};
inline CamFields fill_cam_fields(const MarchArgs &a, uint32_t jitter_seed, uint32_t view_base, double *d_cam, float *d_cam_ray) {
    CamFields f;
    near_plane_extents(a.fov_rad, a.near_plane, a.img_W, a.H, f.near_, f.near_w, f.near_h);   // (img_W = W unless a band)
    f.jitter_seed = jitter_seed; f.view_base = view_base;
    f.d_cam = d_cam; f.d_cam_ray = d_cam_ray;
    f.pose = a.pose; f.fov_v = a.fov_v; f.near_d = a.near_plane; f.aspect = (double)a.img_W / (double)a.H;
    return f;
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

// ---- The free camera: look_from, look_at, up and a per-view fov ------------------------------------------------
// near-plane extents of one view from its own fov, as near_plane_extents forms them on the host: doubles, rounded once
__device__ __forceinline__ void near_plane_extents_dev(float fov_rad, double near_plane, double aspect, float &near_w, float &near_h) {
    const double h = 2.0 * tan((double)fov_rad) * near_plane;
    near_h = (float)h; near_w = (float)(h * aspect);
}

// adjoint of y = normalize(x): (I - y y^T) ybar / |x|
__device__ __forceinline__ f3 normalize_adj(f3 y, float inv_len, f3 ybar) { return f3_scale(inv_len, f3_fma(-dot3(y, ybar), y, ybar)); }

struct PoseGrad { f3 lf, la, up; float fov; };   // d look_from, d look_at, d up, d fov (radians)

// Once per ray, what the pose tail takes from the view and the pixel: look_at and up of pose [views][9], the view's near-plane
// extents (its own with fov_v, else the launch's), the pixel's near-plane coordinates (u, v) (row: within the whole image of
// img_W rows), the jitter draw jit and A = (1 - jit/n)(1 - 0.5/n) of grad t0 = A grad tmin + (1-A) grad tmax.
struct PoseRay { f3 la, up; float u, v, near_w, near_h, jit, A; };
__device__ __forceinline__ PoseRay pose_ray(const float *pose, const float *fov_v, int view, double near_d, double aspect,
                                            float near_w, float near_h, int row, int img_W, int j, int H, int n,
                                            uint32_t jitter_seed, uint32_t hash_view) {
    PoseRay q;
    const float *ps = pose + 9 * view;
    q.la = make_f3(ps[3], ps[4], ps[5]); q.up = make_f3(ps[6], ps[7], ps[8]);
    q.near_w = near_w; q.near_h = near_h;
    if (fov_v) near_plane_extents_dev(fov_v[view], near_d, aspect, q.near_w, q.near_h);
    q.u = ((float)row + 0.5f) / (float)img_W - 0.5f; q.v = ((float)j + 0.5f) / (float)H - 0.5f;
    const float nf = (float)n;
    q.jit = jitter_seed != 0u ? jitter_u(jitter_seed, hash_view, (uint32_t)(row * H + j)) : 0.0f;
    q.A = (1.0f - q.jit / nf) * (1.0f - 0.5f / nf);
    return q;
}

// The pose variant of camera_ray_tail: D8's four sums of one ray -> its ten pose gradients,
//   d theta = [theta in look_from] sP + (d vd / d theta)^T sTG + k_min d tmin / d theta + k_max d tmax / d theta,
// k_min, k_max the caller's weights of the frozen entry and exit faces (the march: s0 A and s0 (1 - A) + s1), with
//   d t / d theta = -([theta is look_from_a] + t d vd_a / d theta) / vd_a   on the face's axis a.
// Both slab rows are a direct look_from term plus a multiple of row a of d vd / d theta, so all ten columns are ONE
// vector-Jacobian product gbar^T (d vd / d theta), gbar = sTG - e_amin k_min tmin / vd_amin - e_amax k_max tmax / vd_amax. It is
// evaluated in reverse through vd = normalize(near view_dir + uw right + vh up'), up' = normalize(right x view_dir),
// right = normalize(view_dir x up), view_dir = normalize(look_at - look_from), uw = u near_w, vh = v near_h,
// near_h = 2 near tan(fov), near_w = near_h img_W / H: twelve 3-vectors, where the three 3x3 Jacobians and the fov column
// carried forward are thirty columns (the fixed camera's ray_dir_jacobian keeps its forward form and its bits).
__device__ __forceinline__ PoseGrad pose_ray_grad(f3 lf, const PoseRay &q, f3 vd, float near_, f3 sP, f3 sTG, float k_min,
                                                  float k_max) {
    const f3 la = q.la, up0 = q.up;
    const float u = q.u, v = q.v, near_w = q.near_w, near_h = q.near_h;
    const SlabFaces sf = slab_faces(lf, vd);   // the faces the forward picked
    const int amin = sf.amin, amax = sf.amax;
    const float tmin = sf.tmin, tmax = sf.tmax, ivmin = sf.ivmin, ivmax = sf.ivmax;
    const f3 emin = make_f3(amin == 0 ? 1.0f : 0.0f, amin == 1 ? 1.0f : 0.0f, amin == 2 ? 1.0f : 0.0f);
    const f3 emax = make_f3(amax == 0 ? 1.0f : 0.0f, amax == 1 ? 1.0f : 0.0f, amax == 2 ? 1.0f : 0.0f);
    const float cmin = -k_min * ivmin, cmax = -k_max * ivmax;
    PoseGrad g;
    g.lf = f3_fma(cmax, emax, f3_fma(cmin, emin, sP));
    const f3 gbar = f3_fma(cmax * tmax, emax, f3_fma(cmin * tmin, emin, sTG));

    // the camera model forward (ray_setup.hip's), then its adjoint
    const f3 a = make_f3(la.x - lf.x, la.y - lf.y, la.z - lf.z);
    const float ia = inv_norm3(a);
    const f3 vdir = f3_scale(ia, a);
    const f3 c = cross_f3(vdir, up0);
    const float ic = inv_norm3(c);
    const f3 right = f3_scale(ic, c);
    const f3 d = cross_f3(right, vdir);
    const float id = inv_norm3(d);
    const f3 upp = f3_scale(id, d);
    const float uw = u * near_w, vh = v * near_h;
    const f3 w = f3_add(f3_add(f3_scale(near_, vdir), f3_scale(uw, right)), f3_scale(vh, upp));
    const float iw = inv_norm3(w);
    const f3 wbar = normalize_adj(f3_scale(iw, w), iw, gbar);
    const f3 dbar = normalize_adj(upp, id, f3_scale(vh, wbar));
    const f3 rbar = f3_add(f3_scale(uw, wbar), cross_f3(vdir, dbar));            // d = right x vdir
    const f3 cbar = normalize_adj(right, ic, rbar);
    f3 vbar = f3_add(f3_scale(near_, wbar), cross_f3(dbar, right));
    vbar = f3_add(vbar, cross_f3(up0, cbar));                                    // c = vdir x up
    g.la = normalize_adj(vdir, ia, vbar);
    g.lf = f3_add(g.lf, f3_scale(-1.0f, g.la));
    g.up = cross_f3(cbar, vdir);
    // d near_h / d fov = 2 near (1 + tan^2 fov), tan fov = near_h / (2 near); near_w follows near_h by the aspect near_w / near_h
    const float tn = near_h / (2.0f * near_);
    const float dh = 2.0f * near_ * (1.0f + tn * tn);
    g.fov = dh * (dot3(wbar, right) * u * (near_w / near_h) + dot3(wbar, upp) * v);
    return g;
}

// The end of both pose backwards: camera_reduce for ten components -- its red[3][256] serves four rounds of three, each ending in
// ONE f64 atomic per component and workgroup into d_pose[view][10] (look_from, look_at, up, fov).
__device__ __forceinline__ void pose_reduce(const PoseGrad &g, bool in_img, size_t p, int view, float *d_pose_ray, double *d_pose,
                                            double (&red)[3][256]) {
    const float c[12] = {g.lf.x, g.lf.y, g.lf.z, g.la.x, g.la.y, g.la.z, g.up.x, g.up.y, g.up.z, g.fov, 0.0f, 0.0f};
    if (in_img && d_pose_ray) {
#pragma unroll
        for (int k = 0; k < 10; ++k) d_pose_ray[10 * p + k] = c[k];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        red[0][threadIdx.x] = (double)c[3 * r]; red[1][threadIdx.x] = (double)c[3 * r + 1]; red[2][threadIdx.x] = (double)c[3 * r + 2];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                red[0][threadIdx.x] += red[0][threadIdx.x + w];
                red[1][threadIdx.x] += red[1][threadIdx.x + w];
                red[2][threadIdx.x] += red[2][threadIdx.x + w];
            }
            __syncthreads();
        }
        if ((int)threadIdx.x < (r == 3 ? 1 : 3) && red[threadIdx.x][0] != 0.0)
            atomicAdd(d_pose + 10 * view + 3 * r + threadIdx.x, red[threadIdx.x][0]);
        __syncthreads();   // the next round overwrites red[.][0]
    }
}

// D5 for the ten components: a NaN ray contributes nothing, infinities are clamped
__device__ __forceinline__ PoseGrad pose_finite(PoseGrad g) {
    g.lf = make_f3(finite_or_zero(g.lf.x), finite_or_zero(g.lf.y), finite_or_zero(g.lf.z));
    g.la = make_f3(finite_or_zero(g.la.x), finite_or_zero(g.la.y), finite_or_zero(g.la.z));
    g.up = make_f3(finite_or_zero(g.up.x), finite_or_zero(g.up.y), finite_or_zero(g.up.z));
    g.fov = finite_or_zero(g.fov);
    return g;
}
__device__ __forceinline__ PoseGrad pose_zero() {
    PoseGrad g; g.lf = g.la = g.up = make_f3(0.f, 0.f, 0.f); g.fov = 0.f; return g;
}

}  // namespace dr
