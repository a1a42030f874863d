/*
 * dr_oracle_impl.inc -- CPU restatement of Differender's volume_raycaster hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under differender_amd/ may include, link or call this.
 * PARITY UNPINNED: the reference (nanovis/Differender, differender/volume_raycaster.py, "VR.py")
 * has no tests/golden vectors and cannot be imported (taichi absent), so this restatement is
 * pinned by analytic known-answer tests and f64 finite-difference checks only (tests/test_oracle*.py).
 *
 * This file is included twice by dr_oracle.c, once with REAL=float (the parity oracle: f32
 * arithmetic in the reference's operation order, compiled with -ffp-contract=off) and once with
 * REAL=double (the "mathematical" version used for finite-difference gradient checks).
 *
 * Third-party semantics restated here (taichi / taichi_glsl are un-vendored, unpinned deps):
 *   mix(x,y,a)      = x*(1-a) + y*a
 *   clamp(x,lo,hi)  = min(hi, max(lo, x))
 *   reflect(I,N)    = I - 2*dot(N,I)*N
 *   v.normalized()  = (1/(sqrt(v.v)+0)) * v
 *   dot/norm_sqr    = ((a0*b0 + a1*b1) + a2*b2)
 *   min/max         = NaN-suppressing (fmin/fmax)
 * Arithmetic convention D2: expressions of the form a*b+c inside mix(), dot(), the position and
 * compositing recurrences are evaluated with ONE rounding (fma), as the reference's CUDA backend
 * contracts them; the fma is spelled out here and in the HIP kernels and both are compiled with
 * -ffp-contract=off, so the contraction pattern is fixed instead of compiler-chosen. This matters
 * because the normal is a difference of trilinear taps 2e-3 world units apart: one ulp in a tap is
 * ~6e-5 relative in the normal, i.e. ~1e-5 in the image (the size of the parity tolerance).
 *   AD rules        = max(x,0) passes grad iff 0<x ; min(1,L) passes grad to L iff !(1<L)
 *
 * Field index (i,j,k) <-> world (x,y,z) in [-1,1]^3; volume array is contiguous [VX][VY][VZ].
 * Image arrays are contiguous [W][H] (pixel (i,j) -> i*H + j), RGBA innermost.
 */

#define R_(x) ((REAL)(x))

typedef struct { REAL x, y, z; } SUF(v3);

static inline SUF(v3) SUF(v3_make)(REAL x, REAL y, REAL z) { SUF(v3) r = {x, y, z}; return r; }
static inline REAL SUF(v3_dot)(SUF(v3) a, SUF(v3) b) { return R_FMA(a.z, b.z, R_FMA(a.y, b.y, a.x * b.x)); }
static inline SUF(v3) SUF(v3_cross)(SUF(v3) a, SUF(v3) b) {
    return SUF(v3_make)(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
static inline SUF(v3) SUF(v3_scale)(REAL s, SUF(v3) a) { return SUF(v3_make)(s * a.x, s * a.y, s * a.z); }
static inline SUF(v3) SUF(v3_add)(SUF(v3) a, SUF(v3) b) { return SUF(v3_make)(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline SUF(v3) SUF(v3_sub)(SUF(v3) a, SUF(v3) b) { return SUF(v3_make)(a.x - b.x, a.y - b.y, a.z - b.z); }
/* taichi Vector.normalized(eps=0): invlen = 1/(norm+eps); return invlen*self */
static inline SUF(v3) SUF(v3_normalized)(SUF(v3) a) {
    REAL inv = R_(1.0) / (R_SQRT(SUF(v3_dot)(a, a)) + R_(0.0));
    return SUF(v3_scale)(inv, a);
}
static inline REAL SUF(mix)(REAL x, REAL y, REAL a) { return R_FMA(y, a, x * (R_(1.0) - a)); }

/* ---- jitter RNG: counter-based hash shared bit-for-bit with the HIP kernels (replaces ti.random,
 * VR.py:255, which is a per-thread stateful generator that cannot be reproduced). ---- */
static inline uint32_t SUF(dr_hash_u32)(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
static inline REAL SUF(dr_jitter_u)(uint32_t seed, uint32_t view, uint32_t pix) {
    uint32_t h = SUF(dr_hash_u32)(seed ^ 0x9E3779B9U);
    h = SUF(dr_hash_u32)(h ^ (view * 0x85EBCA6BU + 0xC2B2AE35U));
    h = SUF(dr_hash_u32)(h ^ pix);
    return R_(h >> 8) * R_(1.0 / 16777216.0); /* U[0,1), 24 bits */
}

/* ---- VR.py:7-21 low_high_frac ---- */
static inline void SUF(low_high_frac)(REAL x, int *lo, int *hi, REAL *fr) {
    x = R_FMAX(x, R_(0.0));
    REAL low = R_FLOOR(x);
    *fr = x - low;
    *lo = (int)low;
    *hi = (int)(low + R_(1.0));
}

/* ---- VR.py:28-53 get_entry_exit_points (box = [-1,1]^3) ---- */
static inline void SUF(entry_exit)(SUF(v3) o, SUF(v3) d, REAL *tmin_o, REAL *tmax_o, int *hit_o) {
    REAL fx = R_(1.0) / d.x, fy = R_(1.0) / d.y, fz = R_(1.0) / d.z;
    REAL t1 = (R_(-1.0) - o.x) * fx, t2 = (R_(1.0) - o.x) * fx;
    REAL t3 = (R_(-1.0) - o.y) * fy, t4 = (R_(1.0) - o.y) * fy;
    REAL t5 = (R_(-1.0) - o.z) * fz, t6 = (R_(1.0) - o.z) * fz;
    REAL tmin = R_FMAX(R_FMAX(R_FMIN(t1, t2), R_FMIN(t3, t4)), R_FMIN(t5, t6));
    REAL tmax = R_FMIN(R_FMIN(R_FMAX(t1, t2), R_FMAX(t3, t4)), R_FMAX(t5, t6));
    int hit = 1;
    if (tmax < R_(0.0) || tmin > tmax) hit = 0;
    *tmin_o = tmin; *tmax_o = tmax; *hit_o = hit;
}

/* ---- VR.py:221-259 compute_entry_exit (+ VR.py:127-151 get_ray_direction) ----
 * fov_rad, near arrive as Python doubles; near_h/near_w are formed in double and then rounded
 * (taichi evaluates ti.tan on a Python float with math.tan). vol_diag likewise (VR.py:248-249). */
int SUF(dro_ray_setup)(const REAL *cam, int W, int H, int VX, int VY, int VZ, double fov_rad,
                       double near_d, REAL sr, uint32_t jitter_seed, uint32_t view,
                       REAL *entry, REAL *exit_, REAL *rays, int32_t *nsamp) {
    const double near_h_d = 2.0 * tan(fov_rad) * near_d;
    const double near_w_d = near_h_d * ((double)W / (double)H);
    const REAL near_h = R_(near_h_d), near_w = R_(near_w_d), near_ = R_(near_d);
    const REAL vol_diag = R_(sqrt((double)(VX - 1) * (VX - 1) + (double)(VY - 1) * (VY - 1) +
                                  (double)(VZ - 1) * (VZ - 1)));
    const SUF(v3) lf = SUF(v3_make)(cam[0], cam[1], cam[2]);
    const SUF(v3) view_dir = SUF(v3_normalized)(SUF(v3_make)(-lf.x, -lf.y, -lf.z));
    const REAL max_x = R_(W), max_y = R_(H);
    for (int i = 0; i < W; ++i) {
        for (int j = 0; j < H; ++j) {
            REAL x = (R_(i) + R_(0.5)) / max_x;
            REAL y = (R_(j) + R_(0.5)) / max_y;
            REAL u = x - R_(0.5), v = y - R_(0.5);
            SUF(v3) up = SUF(v3_make)(R_(0.0), R_(1.0), R_(0.0));
            SUF(v3) right = SUF(v3_normalized)(SUF(v3_cross)(view_dir, up));
            up = SUF(v3_normalized)(SUF(v3_cross)(right, view_dir));
            SUF(v3) near_m = SUF(v3_add)(lf, SUF(v3_scale)(near_, view_dir));
            SUF(v3) near_pos = SUF(v3_add)(SUF(v3_add)(near_m, SUF(v3_scale)(u * near_w, right)),
                                           SUF(v3_scale)(v * near_h, up));
            SUF(v3) vd = SUF(v3_normalized)(SUF(v3_sub)(near_pos, lf));
            REAL tmin, tmax; int hit;
            SUF(entry_exit)(lf, vd, &tmin, &tmax, &hit);
            REAL ray_len = tmax - tmin;
            REAL n_samples = R_(hit) * (R_FLOOR(sr * ray_len * vol_diag) + R_(1.0));
            if (jitter_seed != 0u) {
                REAL uu = SUF(dr_jitter_u)(jitter_seed, view, (uint32_t)(i * H + j));
                tmin += uu * ray_len / n_samples;
            }
            size_t p = (size_t)i * H + j;
            entry[p] = tmin; exit_[p] = tmax;
            rays[3 * p + 0] = vd.x; rays[3 * p + 1] = vd.y; rays[3 * p + 2] = vd.z;
            /* float -> int as the GPUs do it (CUDA cvt.rzi.s32.f32, AMD v_cvt_i32_f32): NaN -> 0, saturating. A C cast of
             * NaN is undefined (x86 gives INT_MIN). NaN arises for a ray parallel to a slab it lies outside of: both
             * slab distances are the same infinity, the hit test passes and ray_len = inf - inf. */
            nsamp[p] = (n_samples != n_samples) ? 0 : (n_samples >= R_(2147483520.0) ? INT32_MAX : (int32_t)n_samples);
        }
    }
    return 0;
}

/* ---- volume access ---- */
typedef struct {
    const REAL *vol; int VX, VY, VZ; REAL scx, scy, scz; /* scale = shape - 1 - 1e-4 (double -> REAL) */
    const REAL *tf; int R; REAL tf_len;
    SUF(v3) cam; SUF(v3) light_pos;
    REAL sr, inv_sr;
} SUF(scene);

typedef struct { int x0, x1, y0, y1, z0, z1; REAL fx, fy, fz; } SUF(cell);

/* VR.py:153-189 sample_volume_trilinear: cell lookup part */
static inline void SUF(tri_cell)(const SUF(scene) *sc, SUF(v3) pos, SUF(cell) *c) {
    REAL px = R_FMIN(R_(1.0), R_FMAX(R_(0.0), R_FMA(R_(0.5), pos.x, R_(0.5)))) * sc->scx;
    REAL py = R_FMIN(R_(1.0), R_FMAX(R_(0.0), R_FMA(R_(0.5), pos.y, R_(0.5)))) * sc->scy;
    REAL pz = R_FMIN(R_(1.0), R_FMAX(R_(0.0), R_FMA(R_(0.5), pos.z, R_(0.5)))) * sc->scz;
    SUF(low_high_frac)(px, &c->x0, &c->x1, &c->fx);
    SUF(low_high_frac)(py, &c->y0, &c->y1, &c->fy);
    SUF(low_high_frac)(pz, &c->z0, &c->z1, &c->fz);
    if (c->x1 > sc->VX - 1) c->x1 = sc->VX - 1;
    if (c->y1 > sc->VY - 1) c->y1 = sc->VY - 1;
    if (c->z1 > sc->VZ - 1) c->z1 = sc->VZ - 1;
    /* defined-domain guard (reference would read out of bounds): keep lo inside the array */
    if (c->x0 > sc->VX - 1) c->x0 = sc->VX - 1;
    if (c->y0 > sc->VY - 1) c->y0 = sc->VY - 1;
    if (c->z0 > sc->VZ - 1) c->z0 = sc->VZ - 1;
}
#define VIDX(sc, i, j, k) (((size_t)(i) * (sc)->VY + (j)) * (sc)->VZ + (k))
static inline REAL SUF(tri_eval)(const SUF(scene) *sc, const SUF(cell) *c) {
    const REAL *V = sc->vol;
    REAL v000 = V[VIDX(sc, c->x0, c->y0, c->z0)], v100 = V[VIDX(sc, c->x1, c->y0, c->z0)];
    REAL a = SUF(mix)(v000, v100, c->fx);
    REAL v010 = V[VIDX(sc, c->x0, c->y1, c->z0)], v110 = V[VIDX(sc, c->x1, c->y1, c->z0)];
    REAL b = SUF(mix)(v010, v110, c->fx);
    REAL zl = SUF(mix)(a, b, c->fy);
    REAL v001 = V[VIDX(sc, c->x0, c->y0, c->z1)], v101 = V[VIDX(sc, c->x1, c->y0, c->z1)];
    a = SUF(mix)(v001, v101, c->fx);
    REAL v011 = V[VIDX(sc, c->x0, c->y1, c->z1)], v111 = V[VIDX(sc, c->x1, c->y1, c->z1)];
    b = SUF(mix)(v011, v111, c->fx);
    REAL zh = SUF(mix)(a, b, c->fy);
    return SUF(mix)(zl, zh, c->fz);
}
static inline REAL SUF(tri_sample)(const SUF(scene) *sc, SUF(v3) pos) {
    SUF(cell) c; SUF(tri_cell)(sc, pos, &c); return SUF(tri_eval)(sc, &c);
}
/* adjoint of tri_sample w.r.t. the volume: dV[corner] += w_corner * adj */
static inline void SUF(tri_scatter)(const SUF(scene) *sc, SUF(v3) pos, REAL adj, REAL *dV) {
    SUF(cell) c; SUF(tri_cell)(sc, pos, &c);
    REAL gx = R_(1.0) - c.fx, gy = R_(1.0) - c.fy, gz = R_(1.0) - c.fz;
    REAL w[8] = { gx * gy * gz, c.fx * gy * gz, gx * c.fy * gz, c.fx * c.fy * gz,
                  gx * gy * c.fz, c.fx * gy * c.fz, gx * c.fy * c.fz, c.fx * c.fy * c.fz };
    size_t idx[8] = { VIDX(sc, c.x0, c.y0, c.z0), VIDX(sc, c.x1, c.y0, c.z0), VIDX(sc, c.x0, c.y1, c.z0),
                      VIDX(sc, c.x1, c.y1, c.z0), VIDX(sc, c.x0, c.y0, c.z1), VIDX(sc, c.x1, c.y0, c.z1),
                      VIDX(sc, c.x0, c.y1, c.z1), VIDX(sc, c.x1, c.y1, c.z1) };
    for (int q = 0; q < 8; ++q) {
        REAL val = w[q] * adj;
#pragma omp atomic
        dV[idx[q]] += val;
    }
}

/* per-sample forward quantities (VR.py:270-299) */
typedef struct {
    SUF(v3) pos; REAL I; int lo, hi; REAL fr, xtf;
    REAL r, g, b, a; REAL op;
    SUF(v3) grad; REAL gnorm; SUF(v3) nrm; int flat;
    SUF(v3) ld; REAL m, ndl; SUF(v3) rf; REAL q, rdv, spec, Lraw, L;
} SUF(sample);

static inline SUF(v3) SUF(sample_pos)(const SUF(scene) *sc, REAL entry, REAL exit_, SUF(v3) vd, int n, int s) {
    REAL ray_len = exit_ - entry;
    REAL tmin = entry + R_(0.5) * ray_len / R_(n);
    REAL f = R_(s) / R_(n - 1);
    REAL t = SUF(mix)(tmin, exit_, f);
    return SUF(v3_make)(R_FMA(t, vd.x, sc->cam.x), R_FMA(t, vd.y, sc->cam.y), R_FMA(t, vd.z, sc->cam.z));
}

/* intensity + TF + opacity (VR.py:282-285, 205-219) */
static inline void SUF(sample_classify)(const SUF(scene) *sc, SUF(sample) *sm) {
    sm->I = SUF(tri_sample)(sc, sm->pos);
    sm->xtf = sm->I * sc->tf_len;
    SUF(low_high_frac)(sm->xtf, &sm->lo, &sm->hi, &sm->fr);
    if (sm->hi > sc->R - 1) sm->hi = sc->R - 1;
    if (sm->lo > sc->R - 1) sm->lo = sc->R - 1; /* defined-domain guard for I>1 (reference reads OOB) */
    const REAL *t0 = sc->tf + 4 * (size_t)sm->lo, *t1 = sc->tf + 4 * (size_t)sm->hi;
    sm->r = SUF(mix)(t0[0], t1[0], sm->fr); sm->g = SUF(mix)(t0[1], t1[1], sm->fr);
    sm->b = SUF(mix)(t0[2], t1[2], sm->fr); sm->a = SUF(mix)(t0[3], t1[3], sm->fr);
    sm->op = R_(1.0) - R_POW_INV_SR(R_(1.0) - sm->a, sc->inv_sr);
}
/* normal + Phong (VR.py:191-203, 287-299). clampL: diff path clamps lighting to <=1 (VR.py:298). */
static inline void SUF(sample_shade)(const SUF(scene) *sc, SUF(v3) vd, SUF(sample) *sm, int clampL) {
    const REAL delta = R_(1e-3);
    SUF(v3) p = sm->pos;
    REAL dx = SUF(tri_sample)(sc, SUF(v3_make)(p.x + delta, p.y, p.z)) - SUF(tri_sample)(sc, SUF(v3_make)(p.x - delta, p.y, p.z));
    REAL dy = SUF(tri_sample)(sc, SUF(v3_make)(p.x, p.y + delta, p.z)) - SUF(tri_sample)(sc, SUF(v3_make)(p.x, p.y - delta, p.z));
    REAL dz = SUF(tri_sample)(sc, SUF(v3_make)(p.x, p.y, p.z + delta)) - SUF(tri_sample)(sc, SUF(v3_make)(p.x, p.y, p.z - delta));
    sm->grad = SUF(v3_make)(dx, dy, dz);
    sm->gnorm = R_SQRT(SUF(v3_dot)(sm->grad, sm->grad));
    sm->flat = !(sm->gnorm > R_(0.0));
    sm->ld = SUF(v3_normalized)(SUF(v3_sub)(p, sc->light_pos));
    if (sm->flat) {
        /* Reference: 0/0 -> NaN normal; NaN-suppressing max() then yields ndl = rdv = 0 (SURVEY H3).
         * Stated here explicitly so the result does not depend on NaN propagation details. */
        sm->nrm = SUF(v3_make)(R_(0.0), R_(0.0), R_(0.0));
        sm->m = R_(0.0); sm->ndl = R_(0.0); sm->rf = sm->ld; sm->q = R_(0.0); sm->rdv = R_(0.0);
    } else {
        sm->nrm = SUF(v3_scale)(R_(1.0) / (sm->gnorm + R_(0.0)), sm->grad);
        sm->m = SUF(v3_dot)(sm->nrm, sm->ld);
        sm->ndl = R_FMAX(sm->m, R_(0.0));
        REAL two_m = R_(2.0) * SUF(v3_dot)(sm->nrm, sm->ld);
        sm->rf = SUF(v3_make)(R_FMA(-two_m, sm->nrm.x, sm->ld.x), R_FMA(-two_m, sm->nrm.y, sm->ld.y), R_FMA(-two_m, sm->nrm.z, sm->ld.z));
        sm->q = -SUF(v3_dot)(sm->rf, vd); /* r.dot(-vd): negation is exact */
        sm->rdv = R_FMAX(sm->q, R_(0.0));
    }
    sm->spec = R_(0.3) * R_POW(sm->rdv, R_(32.0));
    sm->Lraw = R_FMA(R_(0.8), sm->ndl, sm->spec) + R_(0.4);
    sm->L = clampL ? R_FMIN(R_(1.0), sm->Lraw) : sm->Lraw;
}

static void SUF(scene_init)(SUF(scene) *sc, const REAL *vol, int VX, int VY, int VZ, const REAL *tf, int R,
                            const REAL *cam, REAL sr) {
    sc->vol = vol; sc->VX = VX; sc->VY = VY; sc->VZ = VZ;
    sc->scx = R_((double)VX - 1.0 - 1e-4); sc->scy = R_((double)VY - 1.0 - 1e-4); sc->scz = R_((double)VZ - 1.0 - 1e-4);
    sc->tf = tf; sc->R = R; sc->tf_len = R_(R - 1);
    sc->cam = SUF(v3_make)(cam[0], cam[1], cam[2]);
    sc->light_pos = SUF(v3_add)(sc->cam, SUF(v3_make)(R_(0.0), R_(1.0), R_(0.0)));
    sc->sr = sr; sc->inv_sr = R_(1.0) / sr;
}

/* ---- VR.py:261-306 raycast + :363-372 get_final_image (mode 0), and
 *      VR.py:308-361 raycast_nondiff + get_final_image_nondiff (mode 1). Tape-free: only the running
 *      tape value is kept. H1: tape[-1] := 0. H2: diff path marches min(n, S) samples.
 *      steps[p] = number of samples that passed the early-termination test (= valid_sample_step_count-1
 *      in diff mode, VR.py:303,381). */
int SUF(dro_march_fwd)(const REAL *vol, int VX, int VY, int VZ, const REAL *tf, int R, const REAL *cam,
                       const REAL *entry, const REAL *exit_, const REAL *rays, const int32_t *nsamp,
                       int W, int H, int S, REAL sr, int mode, REAL *out_rgba, int32_t *steps) {
    SUF(scene) sc; SUF(scene_init)(&sc, vol, VX, VY, VZ, tf, R, cam, sr);
    const long NP = (long)W * H;
#pragma omp parallel for schedule(dynamic, 64)
    for (long p = 0; p < NP; ++p) {
        int n = nsamp[p];
        SUF(v3) vd = SUF(v3_make)(rays[3 * p], rays[3 * p + 1], rays[3 * p + 2]);
        REAL C0 = 0, C1 = 0, C2 = 0, A = 0; int cnt = 0;
        int nmarch = (mode == 0 && n > S) ? S : n;
        for (int s = 0; s < nmarch; ++s) {
            if (!(A < R_(0.99))) break; /* remaining iterations only copy the tape (VR.py:305-306) */
            SUF(sample) sm;
            sm.pos = SUF(sample_pos)(&sc, entry[p], exit_[p], vd, n, s);
            SUF(sample_classify)(&sc, &sm);
            ++cnt;
            if (mode == 1 && !(sm.a > R_(1e-3))) continue;
            SUF(sample_shade)(&sc, vd, &sm, mode == 0);
            REAL T = R_(1.0) - A;
            C0 = R_FMA(T, sm.L * sm.r * sm.op, C0); /* light_color = 1 (VR.py:95) */
            C1 = R_FMA(T, sm.L * sm.g * sm.op, C1);
            C2 = R_FMA(T, sm.L * sm.b * sm.op, C2);
            A = R_FMA(T, sm.op, A);
        }
        if (mode == 1) { C0 = R_FMIN(R_(1.0), C0); C1 = R_FMIN(R_(1.0), C1); C2 = R_FMIN(R_(1.0), C2); A = R_FMIN(R_(1.0), A); }
        out_rgba[4 * p + 0] = C0; out_rgba[4 * p + 1] = C1; out_rgba[4 * p + 2] = C2; out_rgba[4 * p + 3] = A;
        if (steps) steps[p] = cnt;
    }
    return 0;
}

#ifdef DRO_ACC64
/* ---- the same march with C and A carried in double (f32 instantiation only): the samples, their shading and each
 * contribution T * (L * rgb * op) are dro_march_fwd's float32 values; only the running composite is not rounded to float
 * after every sample. What summing a segment's contributions first (the brick kernels' partials) comes close to: the gap to
 * dro_march_fwd is the sequential float32 rounding the kernels must bound (DESIGN.md D4). The termination test is the
 * reference's A < 0.99f. */
int dro_march_fwd_f32_acc64(const float *vol, int VX, int VY, int VZ, const float *tf, int R, const float *cam,
                            const float *entry, const float *exit_, const float *rays, const int32_t *nsamp,
                            int W, int H, int S, float sr, int mode, float *out_rgba, int32_t *steps) {
    SUF(scene) sc; SUF(scene_init)(&sc, vol, VX, VY, VZ, tf, R, cam, sr);
    const long NP = (long)W * H;
#pragma omp parallel for schedule(dynamic, 64)
    for (long p = 0; p < NP; ++p) {
        int n = nsamp[p];
        SUF(v3) vd = SUF(v3_make)(rays[3 * p], rays[3 * p + 1], rays[3 * p + 2]);
        double C0 = 0, C1 = 0, C2 = 0, A = 0; int cnt = 0;
        int nmarch = (mode == 0 && n > S) ? S : n;
        for (int s = 0; s < nmarch; ++s) {
            if (!(A < (double)0.99f)) break;
            SUF(sample) sm;
            sm.pos = SUF(sample_pos)(&sc, entry[p], exit_[p], vd, n, s);
            SUF(sample_classify)(&sc, &sm);
            ++cnt;
            if (mode == 1 && !(sm.a > 1e-3f)) continue;
            SUF(sample_shade)(&sc, vd, &sm, mode == 0);
            const double T = 1.0 - A;
            C0 += T * (double)(sm.L * sm.r * sm.op);
            C1 += T * (double)(sm.L * sm.g * sm.op);
            C2 += T * (double)(sm.L * sm.b * sm.op);
            A += T * (double)sm.op;
        }
        if (mode == 1) { C0 = fmin(1.0, C0); C1 = fmin(1.0, C1); C2 = fmin(1.0, C2); A = fmin(1.0, A); }
        out_rgba[4 * p + 0] = (float)C0; out_rgba[4 * p + 1] = (float)C1; out_rgba[4 * p + 2] = (float)C2;
        out_rgba[4 * p + 3] = (float)A;
        if (steps) steps[p] = cnt;
    }
    return 0;
}
#endif

/* ---- backward of the diff path: what raycast.grad + get_final_image.grad (VR.py:460-461,470-471)
 * compute, written as an explicit reverse sweep over a per-ray tape of prefix alphas (the reference's
 * render_tape, VR.py:82,102-103, restricted to what the adjoint needs).
 * d_vol [VX][VY][VZ] and d_tf [R][4] are ACCUMULATED into (caller zeroes). Either may be NULL.
 * Deviation D1 (SURVEY H3): where the reference would inject NaN (flat normal), the normal-path
 * gradient is defined as 0. */
int SUF(dro_march_bwd)(const REAL *vol, int VX, int VY, int VZ, const REAL *tf, int R, const REAL *cam,
                       const REAL *entry, const REAL *exit_, const REAL *rays, const int32_t *nsamp,
                       int W, int H, int S, REAL sr, const REAL *grad_out, REAL *d_vol, REAL *d_tf) {
    SUF(scene) sc; SUF(scene_init)(&sc, vol, VX, VY, VZ, tf, R, cam, sr);
    const long NP = (long)W * H;
    const REAL delta = R_(1e-3);
    /* d_tf: thousands of contributions land on a few texels, so f32 atomics in thread order would make the result
     * depend on the OpenMP schedule at the 1e-5 level. Each thread sums its share in double; the shares are combined
     * in double as well and rounded once. (d_vol: a few hundred contributions per voxel, f32 atomics as in the
     * reference.) */
    double *dtf_acc = d_tf ? (double *)calloc((size_t)R * 4, sizeof(double)) : NULL;
#pragma omp parallel
    {
        REAL *tapeA = (REAL *)malloc(sizeof(REAL) * (size_t)(S > 0 ? S : 1));
        double *dtf_loc = d_tf ? (double *)calloc((size_t)R * 4, sizeof(double)) : NULL;
#pragma omp for schedule(dynamic, 64)
        for (long p = 0; p < NP; ++p) {
            int n = nsamp[p];
            int nmarch = n > S ? S : n;
            if (nmarch <= 0) continue;
            SUF(v3) vd = SUF(v3_make)(rays[3 * p], rays[3 * p + 1], rays[3 * p + 2]);
            /* forward sweep: record A_{s-1} for each live sample */
            REAL A = 0; int live = 0;
            for (int s = 0; s < nmarch; ++s) {
                if (!(A < R_(0.99))) break;
                SUF(sample) sm;
                sm.pos = SUF(sample_pos)(&sc, entry[p], exit_[p], vd, n, s);
                SUF(sample_classify)(&sc, &sm);
                tapeA[s] = A;
                A = R_FMA(R_(1.0) - A, sm.op, A);
                ++live;
            }
            const REAL gC0 = grad_out[4 * p], gC1 = grad_out[4 * p + 1], gC2 = grad_out[4 * p + 2];
            REAL Abar = grad_out[4 * p + 3];
            for (int s = live - 1; s >= 0; --s) {
                SUF(sample) sm;
                sm.pos = SUF(sample_pos)(&sc, entry[p], exit_[p], vd, n, s);
                SUF(sample_classify)(&sc, &sm);
                SUF(sample_shade)(&sc, vd, &sm, 1);
                REAL T = R_(1.0) - tapeA[s];
                REAL sh0 = T * gC0, sh1 = T * gC1, sh2 = T * gC2, sha = T * Abar;
                REAL c0 = sm.L * sm.r * sm.op, c1 = sm.L * sm.g * sm.op, c2 = sm.L * sm.b * sm.op;
                /* adjoint of tape[s-1].w */
                Abar = Abar - ((gC0 * c0 + gC1 * c1 + gC2 * c2) + Abar * sm.op);
                REAL rgbdot = sh0 * sm.r + sh1 * sm.g + sh2 * sm.b;
                REAL op_bar = sha + sm.L * rgbdot;
                REAL r_bar = sm.L * sm.op * sh0, g_bar = sm.L * sm.op * sh1, b_bar = sm.L * sm.op * sh2;
                REAL L_bar = sm.op * rgbdot;
                REAL Lraw_bar = (R_(1.0) < sm.Lraw) ? R_(0.0) : L_bar;
                REAL a_bar = op_bar * sc.inv_sr * R_POW(R_(1.0) - sm.a, sc.inv_sr - R_(1.0));
                if (d_tf) {
                    REAL w0 = R_(1.0) - sm.fr, w1 = sm.fr;
                    REAL cb[4] = { r_bar, g_bar, b_bar, a_bar };
                    for (int k = 0; k < 4; ++k) {
                        REAL v0 = w0 * cb[k], v1 = w1 * cb[k];
                        dtf_loc[4 * (size_t)sm.lo + k] += (double)v0;
                        dtf_loc[4 * (size_t)sm.hi + k] += (double)v1;
                    }
                }
                if (d_vol) {
                    const REAL *t0 = sc.tf + 4 * (size_t)sm.lo, *t1 = sc.tf + 4 * (size_t)sm.hi;
                    REAL fr_bar = (t1[0] - t0[0]) * r_bar + (t1[1] - t0[1]) * g_bar + (t1[2] - t0[2]) * b_bar + (t1[3] - t0[3]) * a_bar;
                    REAL I_bar = (R_(0.0) < sm.xtf) ? fr_bar * sc.tf_len : R_(0.0);
                    SUF(tri_scatter)(&sc, sm.pos, I_bar, d_vol);
                    if (!sm.flat) {
                        REAL ndl_bar = R_(0.8) * Lraw_bar;
                        REAL rdv_bar = R_(0.3) * R_(32.0) * R_POW(sm.rdv, R_(31.0)) * Lraw_bar;
                        REAL q_bar = (R_(0.0) < sm.q) ? rdv_bar : R_(0.0);
                        SUF(v3) rf_bar = SUF(v3_make)(-vd.x * q_bar, -vd.y * q_bar, -vd.z * q_bar);
                        REAL m_bar = ((R_(0.0) < sm.m) ? ndl_bar : R_(0.0)) - R_(2.0) * SUF(v3_dot)(sm.nrm, rf_bar);
                        SUF(v3) n_bar = SUF(v3_add)(SUF(v3_scale)(R_(-2.0) * sm.m, rf_bar), SUF(v3_scale)(m_bar, sm.ld));
                        REAL nn = SUF(v3_dot)(sm.nrm, n_bar);
                        REAL inv = R_(1.0) / sm.gnorm;
                        SUF(v3) g_bar3 = SUF(v3_make)(inv * (n_bar.x - sm.nrm.x * nn), inv * (n_bar.y - sm.nrm.y * nn),
                                                     inv * (n_bar.z - sm.nrm.z * nn));
                        SUF(v3) q = sm.pos;
                        SUF(tri_scatter)(&sc, SUF(v3_make)(q.x + delta, q.y, q.z), g_bar3.x, d_vol);
                        SUF(tri_scatter)(&sc, SUF(v3_make)(q.x - delta, q.y, q.z), -g_bar3.x, d_vol);
                        SUF(tri_scatter)(&sc, SUF(v3_make)(q.x, q.y + delta, q.z), g_bar3.y, d_vol);
                        SUF(tri_scatter)(&sc, SUF(v3_make)(q.x, q.y - delta, q.z), -g_bar3.y, d_vol);
                        SUF(tri_scatter)(&sc, SUF(v3_make)(q.x, q.y, q.z + delta), g_bar3.z, d_vol);
                        SUF(tri_scatter)(&sc, SUF(v3_make)(q.x, q.y, q.z - delta), -g_bar3.z, d_vol);
                    }
                }
            }
        }
        free(tapeA);
        if (dtf_loc) {
#pragma omp critical
            for (int k = 0; k < 4 * R; ++k) dtf_acc[k] += dtf_loc[k];
            free(dtf_loc);
        }
    }
    if (dtf_acc) {
        for (int k = 0; k < 4 * R; ++k) d_tf[k] += (REAL)dtf_acc[k];
        free(dtf_acc);
    }
    return 0;
}

#undef VIDX
#undef R_
