/*
 * differender_hip.h -- C ABI of the MI355X (gfx950) volume-raycaster hot path.
 *
 * The reference (nanovis/Differender) has no FFI: its device code is Taichi-JIT'd Python inside
 * differender/volume_raycaster.py ("VR.py").  Each entry point below replaces one Taichi kernel (or
 * kernel pair) that VR.py's RaycastFunction / Raycaster launch; the reference lines are cited per
 * function.  INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - The library is stateless and re-entrant.  It allocates nothing; every buffer is owned by the
 *    caller (PyTorch on the Python side).  All pointers are DEVICE pointers of ONE device; each call runs on
 *    the device that owns them (hipPointerGetAttributes), whatever the calling thread's current device is --
 *    autograd runs backward on another thread than forward -- and restores the current device afterwards.
 *  - Work is enqueued on `stream` (a hipStream_t passed as void*); no call synchronises.
 *  - Return value: 0 on success, otherwise a hipError_t value (>0) or a DR_E* code (<0);
 *    dr_error_string() renders both.
 *  - Volume = the reference's field index space (i,j,k) of extent (VX,VY,VZ) (VR.py:481 calls it
 *    (W,D,H) of the user's (1,D,H,W) tensor), addressed with ELEMENT strides (sx,sy,sz) so the
 *    permuted view of VR.py:566,571 needs no copy.  vol_dtype: DR_F32 or DR_F16 (fp16 storage,
 *    f32 arithmetic; an extension, the reference is f32-only).
 *  - Image buffers are contiguous [view][W][H](C), exactly the (W,H,4) tensors VR.py:417,438 return.
 *  - n_views > 1 runs that many independent views in one launch (replaces the Python loops of
 *    VR.py:418-426,450-464).  *_view_stride are ELEMENT strides between views; 0 shares the buffer
 *    between all views (a shared volume then receives ONE accumulated d_vol).
 */
#ifndef DIFFERENDER_HIP_H
#define DIFFERENDER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_ABI_VERSION 9

enum { DR_F32 = 0, DR_F16 = 1 };
enum { DR_MODE_DIFF = 0, DR_MODE_NONDIFF = 1 };
/* kernel variant selector: AUTO picks the fastest validated kernels for the problem (brick-centric, one lane
 * per sample); BASELINE forces the plain one-lane-per-ray kernels (kept for differential testing and as the
 * fallback for problems the fast kernels do not serve). */
enum { DR_VARIANT_AUTO = 0, DR_VARIANT_BASELINE = 1 };
/* Caller hints for dr_march_fwd[_rows], OR-ed into `variant` (bits 8 and up; the variant proper is the low byte). A hint
 * only chooses between ways of computing the SAME result -- a wrong one costs time, never correctness:
 *   DR_HINT_NO_EARLY_TERMINATION  "no ray can reach alpha 0.99 with this TF": the launches of the alpha pre-pass (which the
 *       device would gate off anyway, once it has looked at the TF's largest alpha) are not issued at all. The device still
 *       checks; if the hint was wrong, every ray of the view is marched whole by the per-ray kernels (exact early termination,
 *       10-40 x slower) and workspace header word 8 counts the views it happened to.
 *   DR_HINT_EARLY_TERMINATION     "many rays terminate early": the alpha pre-pass runs front to back in groups of brick
 *       layers also below sampling rate 3, so that later groups skip the rays that are already opaque.
 * differender_amd.functional derives both from the TF tensor (largest alpha, cached per tensor version, no host sync).
 *   DR_COUNT_EVALUATED (dr_march_fwd[_rows] AND dr_march_bwd[_rows]; measurement only, bench.py): the brick kernels add up the
 *       samples whose taps they actually EVALUATED -- the work-skipping paths (empty bricks, unlit segments, dead samples behind a
 *       termination point) evaluate nothing for samples that still count as marched -- in 64-bit words of the workspace header:
 *       words 58/59 alpha pre-pass, 60/61 colour march (zeroed by the forward), 62/63 backward (accumulates until the next
 *       forward). One atomic per wave: measurably slower on scenes with many short workgroups, so never set in a timed step. */
/*   DR_TAPE_TF (dr_march_fwd[_rows] with mode DR_MODE_DIFF, and the dr_march_bwd[_rows] of the same inputs with d_vol == NULL):
 *       the caller wants the gradient w.r.t. the transfer function ONLY (BASELINE config C3; the reference's TF optimisation,
 *       examples/taichi_volume_raycaster.py). The forward then leaves a per-SAMPLE tape of (intensity, lighting term) -- 8 B
 *       per marched sample, the two things of a sample the TF gradient needs from the volume -- behind the ordinary workspace
 *       (dr_workspace_bytes_tape), and the backward is a per-ray pass over that tape: no brick is staged, no tap is taken
 *       again. Same results as without the flag (a choice between ways of computing the same thing); the backward checks on
 *       the device that the workspace holds this forward's tape and marches the rays one by one if it does not. A ray with more
 *       samples than the tape reserves per ray (ray buffers made for a higher sampling rate than this call's) never leaves its
 *       slot: forward and backward march it with the per-ray kernels (counted in header word 2). */
enum { DR_HINT_NO_EARLY_TERMINATION = 0x100, DR_HINT_EARLY_TERMINATION = 0x200, DR_COUNT_EVALUATED = 0x400, DR_TAPE_TF = 0x800 };

enum {
    DR_EINVAL = -1,      /* bad argument (null pointer, non-positive extent, unknown enum) */
    DR_EUNSUPPORTED = -2, /* valid request this build cannot serve (e.g. RCCL not present, LDS opt-in refused by the driver) */
    DR_ECOLLECTIVE = -3   /* RCCL reported an error */
};

/* DR_ABI_VERSION for the shipped kernels. A library in which any translation unit was compiled with a timing-only what-if
 * switch (kernels that compute WRONG results on purpose: tools/README.md, csrc/dr_experiment.h) answers -DR_ABI_VERSION, so a
 * loader that checks the version cannot take it for the product by accident. */
int dr_abi_version(void);
/* Bit mask of how this library was built: 0 = the shipped kernels; 1 = a what-if build with wrong results;
 * 2 = diagnostic instrumentation (per-phase clocks / counters in the workspace header; results unchanged, slower);
 * 4 = built WITHOUT one of the two tuned -mllvm compiler flags because this compiler does not know it (csrc/Makefile's probe:
 *     results unchanged, kernels a few per cent slower -- a bench line from such a build says so). */
int dr_build_flags(void);
const char *dr_error_string(int code);

/* Ray generation + box clipping + sample count + jitter.
 * Replaces VolumeRaycaster.compute_entry_exit (VR.py:221-259) incl. get_ray_direction (VR.py:127-151)
 * and get_entry_exit_points (VR.py:28-53).
 *   cam     [n_views][3] camera positions (look_from); the camera looks at the origin (VR.py:233)
 *   fov_rad, near_plane: doubles, as VolumeRaycaster.__init__ holds them (VR.py:77-78)
 *   jitter_seed: 0 = no jitter; otherwise tmin += U[0,1)*len/n with U from a counter-based hash of
 *                (seed, view_base+view, pixel) -- replaces ti.random (VR.py:255) so that forward and
 *                backward see the same offsets
 *   entry, exit_ [n_views][W][H] f32; rays [n_views][W][H][3] f32; nsamp [n_views][W][H] i32 */
int dr_ray_setup(const float *cam, int n_views, int W, int H, int VX, int VY, int VZ,
                 double fov_rad, double near_plane, float sampling_rate,
                 uint32_t jitter_seed, uint32_t view_base,
                 float *entry, float *exit_, float *rays, int32_t *nsamp, void *stream);

/* Scratch memory the fast (brick-centric) march kernels need for n_views views, in bytes; 0 when this
 * problem is only served by the baseline kernels (volume edge > 2000 voxels, or a TF of more than 2030 entries: the
 * brick kernels keep the TF, 16 B per entry, and its double-precision gradient table, 32 B per entry, in LDS beside the
 * brick). The baseline kernels have NO limit on the TF resolution (like the reference): they stage the TF and the
 * double-precision d_tf table in LDS up to 3392 entries, the TF alone up to 10176 (d_tf then accumulates with float
 * atomics on the caller's tensor), and read a larger TF where it lies.
 * The caller allocates it (device memory, 256-byte aligned), passes it to dr_march_fwd and, unchanged,
 * to the dr_march_bwd of the same inputs: the forward leaves the per-segment composite prefixes and the
 * per-ray live sample counts there (the "coarse tape", ~22 B per ray per brick layer; the backward also sums d_tf there, in
 * double, before it hands the totals to the caller's tensor). Replaces the
 * reference's render_tape field (VR.py:82,102-103: 16 B per ray per SAMPLE, twice with its gradient). */
size_t dr_workspace_bytes(int n_views, int W, int H, int VX, int VY, int VZ, int R);
/* ... the same plus the per-sample tape of a DR_TAPE_TF forward: 8 B x min(max_samples, longest possible ray at this sampling
 * rate) per ray (fixed stride: 6.4 GB for a 512^2 view of a 512^3 volume at rate 1 -- the reference's render_tape is 16 B per
 * sample, twice with its gradient: VR.py:82,102-103,116). 0 where dr_workspace_bytes() is 0. */
size_t dr_workspace_bytes_tape(int n_views, int W, int H, int VX, int VY, int VZ, int R, int max_samples, float sampling_rate);

/* Forward march: trilinear sampling, 1-D TF lookup, Phong shading, front-to-back compositing with
 * early termination at A >= 0.99.
 *   mode DR_MODE_DIFF    replaces clear_framebuffer + raycast + get_final_image
 *                        (VR.py:374-382, 261-306, 363-372); marches min(n, max_samples) samples
 *   mode DR_MODE_NONDIFF replaces raycast_nondiff + get_final_image_nondiff (VR.py:308-361)
 *   tf      [n_views or 1][R][4] f32
 *   out_rgba [n_views][W][H][4] f32 (overwritten)
 *   steps   [n_views][W][H] i32, nullable: samples that passed the termination test
 *           (= valid_sample_step_count - 1, VR.py:303,381)
 *   fov_rad, near_plane: the pinhole model the ray buffers were generated with (dr_ray_setup); the fast
 *           path uses it to find the pixels a brick projects to. Rays that do not follow the model are
 *           detected (sample-count check) and marched individually, so results stay correct.
 *   workspace: dr_workspace_bytes() bytes, or NULL to force the baseline kernels. */
int dr_march_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                 int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                 const float *tf, int R, int64_t tf_view_stride,
                 const float *cam, const float *entry, const float *exit_, const float *rays,
                 const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                 float sampling_rate, double fov_rad, double near_plane, int mode, int variant,
                 float *out_rgba, int32_t *steps, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the DR_MODE_DIFF march w.r.t. the volume and the transfer function: the hand-derived,
 * tape-free equivalent of get_final_image.grad + raycast.grad (Taichi autodiff, VR.py:460-461,470-471).
 *   grad_out [n_views][W][H][4]  upstream gradient of out_rgba
 *   out_rgba [n_views][W][H][4]  the forward result for the same inputs (saved by the caller)
 *   d_vol    f32, element strides (dsx,dsy,dsz), nullable; ACCUMULATED into (caller zeroes)
 *   d_tf     [n_views or 1][R][4] f32, nullable; ACCUMULATED into (caller zeroes)
 *   workspace: the buffer the forward call of the same inputs filled (fast path), or NULL (baseline).
 * The gradient w.r.t. the camera position is dr_march_bwd_cam (below); the one w.r.t. the sampling rate is not defined
 * (the reference returns None for both, VR.py:465,473-476). */
int dr_march_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                 int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                 const float *tf, int R, int64_t tf_view_stride,
                 const float *cam, const float *entry, const float *exit_, const float *rays,
                 const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                 float sampling_rate, double fov_rad, double near_plane, int variant,
                 const float *grad_out, const float *out_rgba,
                 float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                 float *d_tf, int64_t dtf_view_stride,
                 void *workspace, size_t workspace_bytes, void *stream);

/* Which kernels dr_march_bwd[_rows] would run for these arguments, without running anything (no GPU needed):
 * DR_VARIANT_AUTO = the brick-centric kernels, DR_VARIANT_BASELINE = the plain ones (requested, no workspace, a
 * TF too large for LDS, a volume edge > 2000, strides beyond 32-bit in-box offsets, or more [layer][pixel] slots than
 * 32-bit indices hold: n_views, W, H as in the march call). The ONE function that decides: dr_march_bwd_rows asks it.
 * The brick-centric backward sanitises its gradients itself: a NaN adjoint (NaN pixel of grad_out, NaN voxel)
 * contributes nothing, +-inf and magnitudes beyond 1e30 are clamped per sample, a brick's flush to +-3e38 -- so its
 * caller may skip the torch.nan_to_num of VR.py:463-475. The float atomics that combine bricks, views and work items
 * saturate at +-FLT_MAX (round 4: an addend beyond 1e30 takes a clamping compare-and-swap, atomic_add_sat): where the
 * reference's nan_to_num would turn an overflow into +-3.4e38, so does this path, and no element is ever +-inf or NaN --
 * also when the call is served by the per-ray second pass alone (a stale workspace, a repaired wrong hint): that pass
 * sanitises its adjoints whenever it runs on behalf of the brick-centric backward. The plain kernels (DR_VARIANT_BASELINE)
 * propagate NaN exactly like the reference and rely on nan_to_num. (dsx,dsy,dsz) are ignored if !has_dvol. */
int dr_march_bwd_variant(int n_views, int W, int H, int VX, int VY, int VZ, int R, int64_t sx, int64_t sy, int64_t sz,
                         int64_t dsx, int64_t dsy, int64_t dsz, int has_dvol, int variant, int has_workspace);

/* Image bands: the same three calls for rows [row0, row0 + W) of an image that is img_W rows wide (SURVEY 8(e):
 * "single view => split the image into G tile bands", one band per GPU). All [n_views][W][H] buffers hold the band
 * only; pixel (i, j) of the band is pixel (row0 + i, j) of the image -- same ray, same jitter value, bit for bit, as in
 * a whole-image call. Gradients of the bands add up to the whole image's (all-reduce them like those of views).
 * The plain entry points above are these with img_W = W, row0 = 0. */
int dr_ray_setup_rows(const float *cam, int n_views, int W, int H, int img_W, int row0, int VX, int VY, int VZ,
                      double fov_rad, double near_plane, float sampling_rate,
                      uint32_t jitter_seed, uint32_t view_base,
                      float *entry, float *exit_, float *rays, int32_t *nsamp, void *stream);
int dr_march_fwd_rows(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                      const float *tf, int R, int64_t tf_view_stride,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                      float sampling_rate, double fov_rad, double near_plane, int mode, int variant,
                      float *out_rgba, int32_t *steps, void *workspace, size_t workspace_bytes,
                      int img_W, int row0, void *stream);
int dr_march_bwd_rows(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                      const float *tf, int R, int64_t tf_view_stride,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                      float sampling_rate, double fov_rad, double near_plane, int variant,
                      const float *grad_out, const float *out_rgba,
                      float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                      float *d_tf, int64_t dtf_view_stride,
                      void *workspace, size_t workspace_bytes, int img_W, int row0, void *stream);

/* Gradient of the DR_MODE_DIFF march w.r.t. the camera position look_from -- a capability the reference lacks
 * (its backward returns None for look_from, VR.py:465,473-476). The camera enters the forward through the ray direction
 * (VR.py:127-151), the slab entry/exit and the jitter offset (VR.py:28-53,245-256), every sample position
 * (VR.py:273-280) and the Phong terms light_pos = look_from + (0,1,0) and r.(-vd) (VR.py:281-297); this is the reverse-mode
 * derivative of that program with its branches frozen: the sample count n, the live samples `steps`, the jitter draw, the
 * slab faces chosen for tmin / tmax, every trilinear cell and every max/min/clamp predicate. Flat normals send no gradient
 * through the normal (D1); single-sample rays contribute nothing (H6); a NaN ray contributes nothing and infinities are clamped
 * (D5). A camera on the y axis is degenerate in the forward already (right = 0) and is not special-cased.
 *   vol ... fov_rad, near_plane: as for dr_march_bwd_rows, the forward's ray buffers (dr_ray_setup_rows) included
 *   jitter_seed, view_base, img_W, row0: those the ray buffers were generated with (the jitter draw is recomputed)
 *   steps    [n_views][W][H] i32: the forward's live samples (dr_march_fwd[_rows]'s `steps`)
 *   grad_out, out_rgba: as for dr_march_bwd_rows
 *   d_cam    [n_views][3] f64, ACCUMULATED into (caller zeroes); one atomic per component per workgroup
 *   d_cam_ray [n_views][W][H][3] f32, nullable: each ray's contribution (overwritten)
 * Bands add up like views: the d_cam of the bands of an image sum to the whole image's. */
int dr_march_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                     int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                     const float *tf, int R, int64_t tf_view_stride,
                     const float *cam, const float *entry, const float *exit_, const float *rays,
                     const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                     float sampling_rate, double fov_rad, double near_plane,
                     uint32_t jitter_seed, uint32_t view_base, int img_W, int row0,
                     const int32_t *steps, const float *grad_out, const float *out_rgba,
                     double *d_cam, float *d_cam_ray, void *stream);

/* The free camera: look_at, up and a per-view field of view beside look_from, and their gradients -- what the
 * reference's camera fixes (it looks at the origin, up = +y, one scalar fov: VR.py:127-151).
 *   view_dir = normalize(look_at - look_from), right = normalize(view_dir x up), up' = normalize(right x view_dir),
 *   near_h = 2 tan(fov) near, near_w = near_h img_W / H, vd = normalize(near view_dir + u near_w right + v near_h up');
 * slab clipping, sample count and jitter are dr_ray_setup_rows'. The light stays at look_from + (0,1,0) in world space: it does
 * not follow `up`. `up` parallel to view_dir is degenerate (right = 0), as the fixed camera on the y axis is, and is not
 * special-cased; a fov outside (0, pi/2) is not checked (the values live on the device: no synchronisation).
 *   pose   [n_views][9] f32: look_from, look_at, up of every view. NULL: the fixed camera -- each entry below is then the
 *          entry it is named after, which in turn is this one with pose = fov_v = NULL.
 *   fov_v  [n_views] f32, radians, nullable (only with a pose): NULL takes fov_rad for every view, through the host's double
 *          arithmetic, so that the default pose (look_at 0, up +y) gives dr_ray_setup_rows' buffers bit for bit; given, the
 *          extents are formed per view on the device in double and rounded once.
 * dr_ray_setup_pose_rows reads look_from from the pose (cam may be NULL then). The march entries read `cam` [n_views][3] as the
 * ray origin as ever: it holds the pose's look_from rows. They hand the pose to the brick-centric kernels, whose pixel
 * rectangles and line pre-test follow the camera's basis; without it the rays of a panned or rolled camera would fail the
 * sample-count check and be marched one by one (correct, but off the fast path). A backward takes the pose of its forward. */
int dr_ray_setup_pose_rows(const float *cam, int n_views, int W, int H, int img_W, int row0, int VX, int VY, int VZ,
                           double fov_rad, double near_plane, float sampling_rate,
                           uint32_t jitter_seed, uint32_t view_base,
                           float *entry, float *exit_, float *rays, int32_t *nsamp,
                           const float *pose, const float *fov_v, void *stream);
int dr_march_fwd_rows_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                           int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                           const float *tf, int R, int64_t tf_view_stride,
                           const float *cam, const float *entry, const float *exit_, const float *rays,
                           const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                           float sampling_rate, double fov_rad, double near_plane, int mode, int variant,
                           float *out_rgba, int32_t *steps, void *workspace, size_t workspace_bytes,
                           int img_W, int row0, const float *pose, const float *fov_v, void *stream);
int dr_march_bwd_rows_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                           int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                           const float *tf, int R, int64_t tf_view_stride,
                           const float *cam, const float *entry, const float *exit_, const float *rays,
                           const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                           float sampling_rate, double fov_rad, double near_plane, int variant,
                           const float *grad_out, const float *out_rgba,
                           float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                           float *d_tf, int64_t dtf_view_stride,
                           void *workspace, size_t workspace_bytes, int img_W, int row0,
                           const float *pose, const float *fov_v, void *stream);

/* Gradient of the DR_MODE_DIFF march w.r.t. the pose: dr_march_bwd_cam for ten parameters, from the same per-ray sums and with
 * the same frozen branches, H6, D1 and D5.
 *   pose (not NULL), fov_v: those of the forward; the other arguments as for dr_march_bwd_cam
 *   d_pose     [n_views][10] f64, ACCUMULATED into (caller zeroes): d look_from, d look_at, d up, d fov (per radian; with
 *              fov_v NULL the gradient w.r.t. fov_rad); one atomic per component per workgroup
 *   d_pose_ray [n_views][W][H][10] f32, nullable: each ray's contribution (overwritten) */
int dr_march_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                      const float *tf, int R, int64_t tf_view_stride,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples,
                      float sampling_rate, double fov_rad, double near_plane,
                      uint32_t jitter_seed, uint32_t view_base, int img_W, int row0,
                      const int32_t *steps, const float *grad_out, const float *out_rgba,
                      const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray, void *stream);

/* The one exchange step of the path when views (or image bands) are sharded over the GPUs of a node: an in-place float32
 * SUM all-reduce of the shared gradients over RCCL / xGMI (the reference is single-device and has no
 * counterpart). For hosts without torch.distributed -- the Python package itself uses torch's "nccl" backend, which is the
 * same RCCL. RCCL is dlopen()ed on first use (DR_EUNSUPPORTED if absent); a communicator is an opaque ncclComm_t.
 *   one process per GPU:   rank 0 calls dr_comm_unique_id(id) and ships the 128 bytes to its peers by any means;
 *                          every rank: hipSetDevice(its GPU); dr_comm_init_rank(&comm, n_ranks, id, rank)
 *   one process, n GPUs:   dr_comm_init_all(comms, n, devices) (devices NULL = 0..n-1), then one thread (or a group) per device
 *   per step:              dr_allreduce_gradients_f32(comm, d_vol, n_vol, d_tf, n_tf, stream)   (either may be NULL)
 * d_volume must be ONE dense block of n_vol floats (any axis order: the sum is elementwise), as dr_march_bwd fills it when
 * its strides describe a permutation of a contiguous tensor. The calls are asynchronous on `stream`. */
int dr_comm_unique_id(void *id128);
int dr_comm_init_rank(void **comm, int n_ranks, const void *id128, int rank);
int dr_comm_init_all(void **comms, int n_devices, const int *devices);
int dr_allreduce_f32(void *comm, float *buf, size_t n, void *stream);
int dr_allreduce_gradients_f32(void *comm, float *d_vol, size_t n_vol, float *d_tf, size_t n_tf, void *stream);
int dr_comm_destroy(void *comm);

/* Image loss and its gradient, one pass over the rendered image (the step after the march in an optimisation
 * loop): replaces compute_loss (examples/taichi_volume_raycaster.py:368-373, "EX.py") and the torch mse_loss
 * round trip of EX.py:439-443.
 *   out_rgba, reference  [n] f32 (n = n_views*W*H*4)
 *   grad_out [n] f32, nullable:  (out - ref) * (2*inv_norm)
 *   loss     one f64 on the device, nullable; ACCUMULATED into:  += inv_norm * sum (out - ref)^2
 * inv_norm = 1/n gives torch.nn.functional.mse_loss; 1/(3*W*H) gives EX.py:369-373. */
int dr_mse_loss_grad(const float *out_rgba, const float *reference, int64_t n, float inv_norm,
                     float *grad_out, double *loss, void *stream);

/* The demo's image loss and its gradient: nan_to_num(1 - ssim(res, gt, data_range=1, nonnegative_ssim=True))
 * + mse(res, gt) of examples/test_opt_tf.py:70-72 ("OPT.py"), fused, as differender_amd.utils.losses.ssim2d /
 * dssim_mse_loss define it: an odd win_size Gaussian window (f32 exp, divided by its f32 sum), separable VALID filtering along
 * H then W with a pass skipped when that side is shorter than the window, C1 = (K1 data_range)^2, C2 = (K2 data_range)^2,
 * S_nc the mean of the SSIM map of plane (n, c) (relu'd when flags has DR_SSIM_NONNEGATIVE), ssim its mean over the planes,
 * dssim = 1 - ssim, mse over the full N*C*H*W images. The gradient follows torch's rules: relu passes only where S_nc > 0,
 * nan_to_num only where dssim is finite (a NaN in x gives a NaN loss through the mse and no dssim gradient).
 *   x, y      the render and the target, f32, logical (N, C, H, W) with the element strides strides4[4] (a host array; shared
 *             by x, y and the gradients): a host passes the march's [n_views][W][H][4] output as it lies, with no copy
 *   win_size  odd, <= 31; data_range finite and > 0
 *   stats     [N*C + 3] f64 on the device, WRITTEN (not accumulated): S_nc per plane, then loss, dssim, mse
 *   upstream3 (bwd) 3 f32 on the device: d loss, d dssim, d mse of the caller's objective; NULL = (1, 0, 0)
 *   grad_x    (bwd) [like x] f32, overwritten; grad_y nullable
 * The backward reads only the forward's stats (relu's mask, dssim's finiteness): its gradient is bitwise deterministic. At
 * most three launches per call, no allocation, no host synchronisation. */
enum { DR_SSIM_NONNEGATIVE = 1 };
int dr_dssim_mse_fwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                     double data_range, int win_size, double win_sigma, double K1, double K2, int flags,
                     double *stats, void *stream);
int dr_dssim_mse_bwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                     double data_range, int win_size, double win_sigma, double K1, double K2, int flags,
                     const double *stats, const float *upstream3, float *grad_x, float *grad_y, void *stream);

/* Multi-scale SSIM + MSE image loss and its gradient: nan_to_num(1 - ms_ssim(x, y, data_range, weights))
 * + mse(x, y), fused, as differender_amd.utils.losses.ms_ssim2d / ms_dssim_mse_loss define it (pytorch_msssim.ms_ssim).
 * Level 0 is (x, y); level l+1 is the 2x2 average pool of level l with padding (H_l % 2, W_l % 2), padded zeros counted.
 * Each level takes the SSIM and CS (contrast-structure) maps of dr_dssim_mse_fwd's window; v[l][n][c] is the relu'd per-plane
 * mean of CS for l < levels-1 and of SSIM at the last level; ms[n][c] = prod_l v^weights[l]; dms = 1 - mean(ms); mse over
 * the level-0 images. The gradient follows torch's rules: a plane gets MS gradient only where all its v > 0, and only where
 * dms is finite (nan_to_num).
 *   x, y        f32, logical (N, C, H, W), element strides strides4[4] (a host array, shared by x, y and the gradients;
 *               negative strides allowed: the march's [n_views][W][H][4] output is passed as it lies)
 *   win_size    odd, <= 31, and min(H, W) > 16 (win_size - 1) (pytorch_msssim's condition, whatever `levels`)
 *   weights     host array of `levels` finite weights > 0, 1 <= levels <= DR_MSSSIM_MAX_LEVELS
 *   data_range  finite and > 0
 *   workspace   dr_msssim_workspace_bytes(N, C, H, W, levels, want_grad_y) bytes on the device (want_grad_y: grad_y will be
 *               non-NULL); NULL allowed when that is 0 (levels = 1). Scratch only: nothing is kept in it between calls.
 *   stats       [(levels + 1) N C + 3] f64 on the device, WRITTEN (not accumulated): v[l][n][c], ms[n][c], loss, dms, mse
 *   upstream3   (bwd) 3 f32 on the device: d loss, d dms, d mse of the caller's objective; NULL = (1, 0, 0)
 *   grad_x      (bwd) [like x] f32, overwritten; grad_y nullable
 * The forward is memset + (levels - 1) pooling launches + one tile launch + a finalize; the backward pools again and runs
 * one launch per level with no atomics: its gradient is bitwise deterministic. No allocation, no host synchronisation.
 * Returns 0 for dr_msssim_workspace_bytes' invalid arguments. */
enum { DR_MSSSIM_MAX_LEVELS = 5 };
size_t dr_msssim_workspace_bytes(int N, int C, int H, int W, int levels, int want_grad_y);
int dr_msssim_mse_fwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                      double data_range, int win_size, double win_sigma, double K1, double K2,
                      const double *weights, int levels, void *workspace, double *stats, void *stream);
int dr_msssim_mse_bwd(const float *x, const float *y, int N, int C, int H, int W, const int64_t *strides4,
                      double data_range, int win_size, double win_sigma, double K1, double K2,
                      const double *weights, int levels, const double *stats, const float *upstream3,
                      float *grad_x, float *grad_y, void *workspace, void *stream);

/* 3-D total variation of a volume and its gradient, as differender_amd.utils.losses.tv3d defines it: forward
 * differences d_a along each of the three axes D, H, W of every volume with the last slice repeated (so d_a = 0 at the far edge
 * and an axis of extent 1 contributes nothing; no difference crosses from one volume of the batch into the next), per voxel
 *   DR_TV_L1   |dD| + |dH| + |dW|                       (anisotropic)
 *   DR_TV_ISO  sqrt(dD^2 + dH^2 + dW^2 + eps^2)         (isotropic, Charbonnier; eps > 0 and (float)(eps * eps) > 0, that is
 *                                                        eps >= 3e-23: eps^2 is added in f32, and with 0 a flat voxel's
 *                                                        gradient would be 0 * inf)
 *   DR_TV_SQ   dD^2 + dH^2 + dW^2                       (quadratic, Tikhonov)
 * summed over the voxels of all B volumes. Arithmetic in f32, the sum in f64.
 *   vol       DR_F32 or DR_F16, logical (B, D, H, W) with the int64 element strides strides4[4] (a host array; any order:
 *             Raycaster's permuted (W, D, H) view and d_vol of dr_march_bwd need no copy)
 *   sum       (fwd) one f64 on the device, WRITTEN (not accumulated); a NaN in vol gives a NaN sum
 *   upstream  (bwd) one f32 on the device, d objective / d sum; NULL = 1
 *   grad      (bwd) f32, logical (B, D, H, W) with the strides grad_strides4[4], no two voxels on one element, not aliasing vol:
 *             grad = (accumulate ? grad : 0) + (*upstream) * scale * dTV/dvol, with sign(0) = 0 for DR_TV_L1. accumulate lets a
 *             caller add the regulariser straight into the d_vol of dr_march_bwd.
 * Invalid arguments (null pointers, extents <= 0, an unknown norm or dtype, a non-finite eps or scale, eps <= 0 or
 * (float)(eps * eps) == 0 with DR_TV_ISO) return DR_EINVAL before any HIP call. One launch each (after a memset of sum in the forward), no allocation, no host
 * synchronisation; the backward has no atomics and its gradient is bitwise deterministic. */
enum { DR_TV_L1 = 0, DR_TV_ISO = 1, DR_TV_SQ = 2 };
int dr_tv3d_fwd(const void *vol, int vol_dtype, int B, int D, int H, int W, const int64_t *strides4,
                int norm, double eps, double *sum, void *stream);
int dr_tv3d_bwd(const void *vol, int vol_dtype, int B, int D, int H, int W, const int64_t *strides4,
                int norm, double eps, const float *upstream, float scale, float *grad,
                const int64_t *grad_strides4, int accumulate, void *stream);

/* March with a 2-D (value, gradient-magnitude) transfer function (Levoy 1988, Kniss et al. 2002): a material
 * boundary and the interior of a material of the same value classify differently. Everything is the 1-D march of
 * dr_march_fwd (positions, jitter, sample count, max_samples clip, opacity correction, Phong shading, compositing, early
 * termination at A >= 0.99, the non-differentiable mode's alpha > 1e-3 skip and final clamp) except the classification:
 *   I = trilinear value; (dx, dy, dz) = the six central-difference taps of the shading normal (delta 1e-3);
 *   u = sqrtf(dx^2 + dy^2 + dz^2) * g_scale;  xv = I (RV - 1), xg = u (RG - 1), split into index and fraction on each axis
 *   (negative coordinates clamp to 0, indices to R - 1);
 *   rgba = mix(mix(T[v0][g0], T[v1][g0], fv), mix(T[v0][g1], T[v1][g1], fv), fg)   (value axis first).
 * A (RV, 1) table is bit for bit the 1-D TF of RV entries. One lane per ray (the shape of DR_VARIANT_BASELINE): no workspace,
 * no brick path, no camera gradient.
 *   tf2d     [n_views or 1][RV][RG][4] f32 (RG fastest), tf_view_stride in floats (0 = shared); RV, RG >= 1, RV * RG < 2^31
 *   g_scale  finite, > 0: u = 1 is the last column of the table (differender_amd.tf2d.gradient_scale estimates one)
 *   mode     DR_MODE_DIFF or DR_MODE_NONDIFF; out_rgba and steps as for dr_march_fwd
 * The backward (DR_MODE_DIFF) is the reverse-mode derivative of this program with its branches frozen, hand-derived and
 * tape-free like dr_march_bwd: d_vol through I, through the normal and through u (onto the same six taps; flat samples,
 * |grad| = 0, send nothing through either), d_tf2d by the four bilinear weights. Both are ACCUMULATED (caller zeroes) and
 * nullable; dtf_view_stride 0 = one gradient for a shared table. NaN propagates as in the plain 1-D kernels.
 * Invalid arguments (null required pointers, extents <= 0, RV * RG >= 2^31, a non-finite or non-positive g_scale, an unknown
 * mode or dtype) return DR_EINVAL before any HIP call. */
int dr_march_tf2d_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                      const float *tf2d, int RV, int RG, int64_t tf_view_stride, float g_scale,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                      int mode, float *out_rgba, int32_t *steps, void *stream);
int dr_march_tf2d_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                      const float *tf2d, int RV, int RG, int64_t tf_view_stride, float g_scale,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                      const float *grad_out, const float *out_rgba,
                      float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                      float *d_tf2d, int64_t dtf_view_stride, void *stream);

/* March through a pre-classified ("pre-shaded") RGBA volume: the volume carries colour and opacity per voxel
 * and is composited directly -- no transfer function, no shading. The samples are exactly those of the march, from the buffers
 * of dr_ray_setup (jitter included): m = min(n, max_samples) of them in DR_MODE_DIFF, m = n in DR_MODE_NONDIFF, none for a ray
 * with n <= 1 (pixel 0, steps 0). Per sample: (r, g, b, a) = the trilinear interpolation of the four channels (one cell, the
 * lerps x -> y -> z per channel), op = 1 - (1 - a)^(1 / sampling_rate) (the specified power of dr_march_fwd); while A < 0.99:
 * C_k += (1 - A) c_k op, A += (1 - A) op, sequentially in f32. DR_MODE_NONDIFF counts but does not composite samples with
 * a <= 1e-3 and clamps the pixel to <= 1. Opacities outside [0, 1] are not clamped (NaN propagates as in the plain kernels).
 *   vol      [n_views or 1] x 4 channels x (VX, VY, VZ), DR_F32 or DR_F16, element strides sx, sy, sz, sc (channel) and
 *            vol_view_stride (0 = shared). With sc == 1 and the base pointer, sx, sy, sz and vol_view_stride all multiples of
 *            four elements (an interleaved volume) a voxel is one 16-byte (8-byte) load; the results are the same bits.
 *   out_rgba [n_views][W][H][4] f32; steps [n_views][W][H] int32, the live samples, nullable
 * The backward (DR_MODE_DIFF) is the reverse-mode derivative of this program with n, the live samples and the cells frozen,
 * tape-free like dr_march_bwd; d_vol is f32 with its own strides (dsx, dsy, dsz, dsc, dvol_view_stride; 0 = one gradient summed
 * over the views), ACCUMULATED (caller zeroes); d_vol == NULL returns 0 before any HIP call.
 * Invalid arguments (null required pointers, n_views, W or H <= 0, a volume extent < 2 (as for every march here: dr_ray_setup
 * needs two voxels per axis), max_samples < 1, an unknown mode or dtype, a non-finite or non-positive sampling rate) return
 * DR_EINVAL before any HIP call. */
int dr_march_rgba_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t sc, int64_t vol_view_stride,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                      int mode, float *out_rgba, int32_t *steps, void *stream);
int dr_march_rgba_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                      int64_t sx, int64_t sy, int64_t sz, int64_t sc, int64_t vol_view_stride,
                      const float *cam, const float *entry, const float *exit_, const float *rays,
                      const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                      const float *grad_out, const float *out_rgba,
                      float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dsc, int64_t dvol_view_stride,
                      void *stream);

/* Gradient of the differentiable dr_march_rgba_fwd w.r.t. the camera: dr_march_bwd_cam's chain (D8) for the
 * four-channel volume, without lighting. It is the reverse-mode derivative of ray setup + march with the usual frozen branches:
 * the sample count n, the live samples (`steps` of dr_march_rgba_fwd: m = min(n, max_samples, steps)), the jitter draw, the slab
 * faces picked for entry and exit, every sample's trilinear cell and every clamp predicate. A ray with n <= 1 contributes
 * nothing (H6). A ray whose upstream gradient or pixel is NaN (an alpha > 1 at a rate != 1 makes such a pixel) contributes
 * nothing and infinities are clamped to +-1e30 (D5).
 *   dr_march_rgba_bwd_cam   ACCUMULATES d look_from into d_cam [n_views][3] (f64, caller zeroes) and writes each ray's
 *                           contribution to d_cam_ray [n_views][W][H][3] (f32, nullable, overwritten)
 *   dr_march_rgba_bwd_pose  the same for the free camera: d_pose [n_views][10] = d look_from, d look_at, d up,
 *                           d fov PER RADIAN; d_pose_ray [n_views][W][H][10]; pose [n_views][9] required, fov_v nullable
 * fov_rad, near_plane, jitter_seed, view_base (and pose, fov_v) must be those of the dr_ray_setup[_pose_rows] call that made the
 * buffers. Bands of image rows are not supported: the buffers are whole images. No per-sample or per-ray atomics, and nothing
 * is written to the volume's gradient.
 * Invalid arguments (null required pointers -- steps, d_cam and for _pose pose included --, fov_v without pose, n_views, W or
 * H <= 0, a volume extent < 2, max_samples < 1, an unknown dtype, a non-finite or non-positive sampling rate) return DR_EINVAL
 * before any HIP call. */
int dr_march_rgba_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                          int64_t sx, int64_t sy, int64_t sz, int64_t sc, int64_t vol_view_stride,
                          const float *cam, const float *entry, const float *exit_, const float *rays,
                          const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                          double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                          const int32_t *steps, const float *grad_out, const float *out_rgba,
                          double *d_cam, float *d_cam_ray, void *stream);
int dr_march_rgba_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                           int64_t sx, int64_t sy, int64_t sz, int64_t sc, int64_t vol_view_stride,
                           const float *cam, const float *entry, const float *exit_, const float *rays,
                           const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                           double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                           const int32_t *steps, const float *grad_out, const float *out_rgba,
                           const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray, void *stream);

/* The 1-D TF march with a free light and Phong material. The reference shades every sample with a white light
 * at look_from + (0, 1, 0), ambient 0.4, diffuse 0.8, specular 0.3 and shininess 32 (VR.py:91-95, 281-299); here these are ten
 * parameters per view, and the backward returns their gradients. Everything else is dr_march_fwd's program as its plain kernels
 * run it (VR.py:261-306, 363-372; DR_MODE_NONDIFF: VR.py:308-361): positions, jitter, sample count, max_samples clip, TF
 * lookup, opacity correction, the six normal taps, flat normals (D1), termination at A >= 0.99, the non-differentiable mode's
 * alpha > 1e-3 skip and final clamp. One lane per ray (the shape of DR_VARIANT_BASELINE): no workspace, no brick path, no
 * camera gradient, no bands of rows.
 *   light    [n_views][10] f32 on the device: p (3) the light's WORLD position, lc (3) its colour, ka, kd, ks the ambient,
 *            diffuse and specular weights, sh the shininess
 * Per shaded sample, in f32 with dr_march_fwd's rounding (VR.py:287-299):
 *   ld = normalized(pos - p), m = n.ld, ndl = max(m, 0), rf = ld - 2 m n, q = -rf.vd, rdv = max(q, 0)  (flat normal: ndl = rdv = 0)
 *   P = rdv^sh: five squarings when sh == 32, else the specified power of the opacity correction (D6; 0^sh = 0)
 *   Lraw = fma(kd, ndl, ks P) + ka, L = min(1, Lraw) in DR_MODE_DIFF and Lraw in DR_MODE_NONDIFF
 *   C_k = fma(T, (L c_k op) lc_k, C_k), A = fma(T, op, A)
 * With p = look_from + (0, 1, 0) formed in f32, lc = 1 and 0.4, 0.8, 0.3, 32 the image and `steps` are the bits of dr_march_fwd
 * under DR_VARIANT_BASELINE. A light that coincides with a sample gives NaN, which propagates as in the plain kernels.
 * The backward (DR_MODE_DIFF) is the reverse-mode derivative of this program with dr_march_bwd's frozen branches (the sample
 * count, the termination test re-evaluated as the forward did, every max / min predicate by Taichi's rules), hand-derived and
 * tape-free. d_vol (element strides, dvol_view_stride 0 = one gradient for a shared volume) and d_tf (dtf_view_stride likewise)
 * are f32 and ACCUMULATED (caller zeroes). d_light [n_views][10] is f64 and ACCUMULATED (caller zeroes): ten f32 sums per ray,
 * a NaN sum dropped and infinities clamped to +-1e30 once per ray, and all ten sums of a ray dropped whose upstream gradient
 * holds a NaN in any channel (D5), f64 per workgroup, one atomic per component and workgroup. d_light_ray [n_views][W][H][10] f32 is OVERWRITTEN with each ray's contribution. Each of the four is nullable and
 * work for an absent one is not done; with all four NULL the call returns 0 before any HIP call.
 * Invalid arguments (null required pointers -- light included --, n_views, W or H <= 0, a volume extent < 2, R < 1,
 * max_samples < 0, a non-positive sampling rate, an unknown mode or dtype; a mode other than DR_MODE_DIFF in the backward)
 * return DR_EINVAL before any HIP call. */
int dr_march_lit_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                     int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                     const float *tf, int R, int64_t tf_view_stride,
                     const float *cam, const float *entry, const float *exit_, const float *rays,
                     const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                     const float *light, int mode, float *out_rgba, int32_t *steps, void *stream);
int dr_march_lit_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                     int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                     const float *tf, int R, int64_t tf_view_stride,
                     const float *cam, const float *entry, const float *exit_, const float *rays,
                     const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                     const float *light, int mode, const float *grad_out, const float *out_rgba,
                     float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                     float *d_tf, int64_t dtf_view_stride, double *d_light, float *d_light_ray, void *stream);

/* Ray-depth moments of the differentiable 1-D TF march: where along a ray the image comes from. The samples are
 * exactly those of dr_march_fwd in DR_MODE_DIFF, from the buffers of dr_ray_setup[_pose_rows] (jitter included). For a ray with
 * n > 1: m = min(n, max_samples) samples at t_s = mix(t0, exit, s/(n-1)), t0 = entry + 0.5 (exit - entry)/n -- the distance from
 * look_from along the unit ray direction, in world units; per sample one trilinear tap, the TF lookup and
 * op = 1 - (1 - a)^(1 / sampling_rate) (the specified power of dr_march_fwd, D6); no normal, no shading. While A < 0.99,
 * sequentially in f32 with T = 1 - A:
 *   M1 = fma(T, t op, M1),  M2 = fma(T, (t t) op, M2),  A = fma(T, op, A).
 * out_moments [n_views][W][H][4] f32 = (M1, M2, 0, A); steps [n_views][W][H] int32 = the live samples, nullable. A ray with
 * n <= 1 gives 0 with 0 steps (H6). A and steps are the bits of dr_march_fwd under DR_VARIANT_BASELINE on the same buffers.
 * M1 / A is the expected depth, M2 / A - (M1 / A)^2 its variance. There is no non-differentiable mode.
 * dr_march_depth_bwd is the reverse-mode derivative with dr_march_bwd's frozen branches (n, the live samples, every cell, the
 * 0 < xtf predicate), tape-free. With g = grad_out (channel 2 is never used) and q_s = g.x t_s + g.y t_s^2 + g.w:
 * op_bar = T_s q_s - suffix / (1 - op_s) (no suffix term for the last live sample), suffix = g . (final - composite after s).
 * d_vol (f32, own element strides, dvol_view_stride 0 = one gradient summed over the views) and d_tf (f32, dtf_view_stride
 * likewise) are ACCUMULATED (caller zeroes). Only the alpha column of d_tf receives anything: the colour columns are not
 * written. NaN propagates as in the plain kernels. d_vol == NULL && d_tf == NULL returns 0 before any HIP call.
 * dr_march_depth_bwd_cam / _bwd_pose: the camera gradient, dr_march_bwd_cam's chain (D8) without lighting and with the direct
 * term of t_s in the integrand; the arguments after sampling_rate are those of dr_march_rgba_bwd_cam / _bwd_pose (`steps` of
 * dr_march_depth_fwd; d_cam [n_views][3] / d_pose [n_views][10] f64 ACCUMULATED, d fov PER RADIAN; per-ray outputs f32,
 * nullable, overwritten). A NaN ray contributes nothing and infinities are clamped to +-1e30 (D5). Whole images only.
 * Invalid arguments (null required pointers, n_views, W or H <= 0, a volume extent < 2, R < 1, max_samples < 1, an unknown
 * dtype, a non-finite or non-positive sampling rate; for the camera entries steps, d_cam, pose for _pose, fov_v without pose)
 * return DR_EINVAL before any HIP call. */
int dr_march_depth_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                       int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                       const float *tf, int R, int64_t tf_view_stride,
                       const float *cam, const float *entry, const float *exit_, const float *rays,
                       const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                       float *out_moments, int32_t *steps, void *stream);
int dr_march_depth_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                       int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                       const float *tf, int R, int64_t tf_view_stride,
                       const float *cam, const float *entry, const float *exit_, const float *rays,
                       const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                       const float *grad_out, const float *out_moments,
                       float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                       float *d_tf, int64_t dtf_view_stride, void *stream);
int dr_march_depth_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                           int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                           const float *tf, int R, int64_t tf_view_stride,
                           const float *cam, const float *entry, const float *exit_, const float *rays,
                           const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                           double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                           const int32_t *steps, const float *grad_out, const float *out_moments,
                           double *d_cam, float *d_cam_ray, void *stream);
int dr_march_depth_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                            int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                            const float *tf, int R, int64_t tf_view_stride,
                            const float *cam, const float *entry, const float *exit_, const float *rays,
                            const int32_t *nsamp, int n_views, int W, int H, int max_samples, float sampling_rate,
                            double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                            const int32_t *steps, const float *grad_out, const float *out_moments,
                            const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray, void *stream);

/* X-ray line-integral and maximum-intensity projections: the two standard projections of a scalar volume beside
 * compositing, differentiable w.r.t. the volume and the camera position. The samples are exactly those of the march, from the
 * ray buffers of dr_ray_setup (jitter included): s < m = min(n, max_samples), pos_s = look_from + mix(t0, exit, s/(n-1)) vd,
 * t0 = entry + 0.5 (exit - entry)/n, mu(pos) the trilinear value (f32 arithmetic also for DR_F16 volumes). A ray with n <= 1
 * gives 0.
 *   DR_PROJ_SUM  out = D sum_{s<m} mu(pos_s), D = (exit - entry)/n in world units of the [-1, 1]^3 box: the line integral (a
 *                constant volume c gives c (exit - entry) for 2 <= n <= max_samples). Sequential f32 sum, times D once.
 *   DR_PROJ_MAX  out = max_{s<m} mu(pos_s); the first maximum wins (strict >), its index goes to arg_max (-1: none; out 0).
 *   vol       as for dr_march_fwd;  out [n_views][W][H] f32;  arg_max [n_views][W][H] int32 (required for MAX, nullable for SUM)
 * The backwards are the reverse-mode derivatives with n, the jitter draw, the slab faces, the trilinear cells and the MAX index
 * frozen. dr_project_bwd ACCUMULATES d_vol (caller zeroes; element strides, dvol_view_stride 0 = one summed gradient for a shared
 * volume): g D w_tap for every SUM sample, g w_tap for the MAX sample. variant DR_VARIANT_AUTO = the windowed SUM backward (a
 * pixel tile's taps of one depth window summed in LDS, then added to d_vol row by row), DR_VARIANT_BASELINE = one lane per ray,
 * global atomics per tap (MAX always). The two differ only in the order of the float additions. d_vol NULL: nothing is
 * requested, 0 is returned before any HIP call.
 * dr_project_bwd_cam ACCUMULATES d look_from into d_cam [n_views][3] (f64) -- the D8 chain of dr_march_bwd_cam without lighting,
 * and for SUM also through D -- and writes each ray's contribution to d_cam_ray [n_views][W][H][3] (nullable). fov_rad,
 * near_plane, jitter_seed and view_base must be those of the dr_ray_setup call that made the buffers.
 * A NaN upstream gradient contributes nothing and infinities are clamped to +-1e30 (D5). Bands of image rows (img_W, row0) are
 * not supported: the buffers are whole images.
 * Invalid arguments (null required pointers, extents <= 0, max_samples < 1, an unknown mode, variant or dtype, MAX without
 * arg_max) return DR_EINVAL before any HIP call. */
enum { DR_PROJ_SUM = 0, DR_PROJ_MAX = 1 };
int dr_project_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                   int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                   const float *cam, const float *entry, const float *exit_, const float *rays,
                   const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode,
                   float *out, int32_t *arg_max, void *stream);
int dr_project_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                   int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                   const float *cam, const float *entry, const float *exit_, const float *rays,
                   const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode,
                   const float *grad_out, const int32_t *arg_max,
                   float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dvol_view_stride,
                   int variant, void *stream);
int dr_project_bwd_cam(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                       int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                       const float *cam, const float *entry, const float *exit_, const float *rays,
                       const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode,
                       double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                       const float *grad_out, const int32_t *arg_max, double *d_cam, float *d_cam_ray, void *stream);

/* dr_project_bwd_cam for the free camera's ten parameters (dr_march_bwd_pose's pose, fov_v, d_pose and d_pose_ray). */
int dr_project_bwd_pose(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                        int64_t sx, int64_t sy, int64_t sz, int64_t vol_view_stride,
                        const float *cam, const float *entry, const float *exit_, const float *rays,
                        const int32_t *nsamp, int n_views, int W, int H, int max_samples, int mode,
                        double fov_rad, double near_plane, uint32_t jitter_seed, uint32_t view_base,
                        const float *grad_out, const int32_t *arg_max,
                        const float *pose, const float *fov_v, double *d_pose, float *d_pose_ray, void *stream);

/* The differentiable 1-D TF march over an arbitrary bundle of rays: dr_march_fwd's DR_MODE_DIFF march and its
 * backwards with a ray as an input -- origins [N][3] and UNIT directions [N][3] f32, used as given, in look_from's world
 * coordinates (the volume fills [-1, 1]^3) -- instead of a pinhole camera's pixel. One volume and one table per call; the light
 * of ray p sits at origins[p] + (0, 1, 0). All per-ray buffers are [N] (out_rgba [N][4]); one lane per ray, so 64 consecutive
 * rays share a wave and the memory coherence of a bundle is the caller's ray order.
 * dr_bundle_setup: dr_ray_setup's slab test, sample count and jitter for the ray as given: for the origin and direction of a
 * dr_ray_setup pixel it writes that pixel's entry, exit and nsamp bit for bit. t_near: -INFINITY = off (the reference's line,
 * which also marches behind an origin inside the box); else tmin = max(tmin, t_near) before the hit test and the sample count
 * (0: a ray). jitter_seed 0 = none; else the draw is that of (jitter_seed, ray_base, p), ray_base playing view_base's part.
 * dr_march_bundle_fwd: out_rgba and steps (nullable) as dr_march_fwd with DR_VARIANT_BASELINE: the rays of a dr_ray_setup view
 * with its camera repeated as the origins give that view's image and steps bit for bit.
 * dr_march_bundle_bwd ACCUMULATES d_vol (element strides dsx, dsy, dsz) and d_tf [R][4] (caller zeroes); either may be NULL,
 * both NULL returns 0 before any HIP call. NaN propagates as in the plain kernels.
 * dr_march_bundle_bwd_rays writes d_origins and d_dirs [N][3] f32 (overwritten): the reverse-mode derivative w.r.t. the origin
 * and w.r.t. the direction as a free 3-vector (normalising it is the caller's, whose chain rule it then is), with the frozen
 * branches of dr_march_bwd_cam (n, `steps` of dr_march_bundle_fwd, the jitter draw, the slab faces, the t_near clamp, the cells,
 * the lighting predicates). t_near, jitter_seed and ray_base must be those of the dr_bundle_setup call that made the buffers. A
 * ray with n <= 1 gets zeros; a NaN ray gets zeros and infinities are clamped to +-1e30 (D5).
 * Invalid arguments (null required pointers, N <= 0, N >= 2^31, a volume extent < 2, R < 1, max_samples < 1, a NaN t_near, an
 * unknown dtype, a non-finite or non-positive sampling rate) return DR_EINVAL before any HIP call; a library linked without
 * these kernels returns DR_EUNSUPPORTED. */
int dr_bundle_setup(const float *origins, const float *dirs, int64_t N, int VX, int VY, int VZ,
                    float sampling_rate, float t_near, uint32_t jitter_seed, uint32_t ray_base,
                    float *entry, float *exit_, int32_t *nsamp, void *stream);
int dr_march_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                        int64_t sx, int64_t sy, int64_t sz, const float *tf, int R,
                        const float *origins, const float *dirs, const float *entry, const float *exit_,
                        const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                        float *out_rgba, int32_t *steps, void *stream);
int dr_march_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                        int64_t sx, int64_t sy, int64_t sz, const float *tf, int R,
                        const float *origins, const float *dirs, const float *entry, const float *exit_,
                        const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                        const float *grad_out, const float *out_rgba,
                        float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, float *d_tf, void *stream);
int dr_march_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                             int64_t sx, int64_t sy, int64_t sz, const float *tf, int R,
                             const float *origins, const float *dirs, const float *entry, const float *exit_,
                             const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                             const int32_t *steps, float t_near, uint32_t jitter_seed, uint32_t ray_base,
                             const float *grad_out, const float *out_rgba,
                             float *d_origins, float *d_dirs, void *stream);

/* X-ray line-integral and maximum-intensity projections of an arbitrary bundle of rays: dr_project_fwd / _bwd
 * with a ray as an input, as the entries above are dr_march_fwd's. origins, dirs, the ray buffers of dr_bundle_setup (at any
 * sampling rate) and N as above; no table. mode is DR_PROJ_SUM or DR_PROJ_MAX; out, grad_out [N] f32, arg_max [N] i32 (written
 * by the forward and read by both backwards for DR_PROJ_MAX, ignored and nullable for DR_PROJ_SUM). The samples are
 * dr_project_fwd's: the rays of a dr_ray_setup view with its camera repeated as the origins give that view's out and arg_max bit
 * for bit.
 * dr_project_bundle_bwd ACCUMULATES d_vol (element strides dsx, dsy, dsz; caller zeroes); d_vol NULL returns 0 before any HIP
 * call. A ray whose g D (SUM) or g (MAX) is NaN contributes nothing, infinities are clamped to +-1e30 (D5). variant
 * DR_VARIANT_BASELINE: one global float atomic per tap; DR_VARIANT_AUTO: for DR_PROJ_SUM, groups of 256 consecutive rays collect
 * their taps per depth window in LDS and flush along d_vol's contiguous axis (a group too incoherent for that finishes per
 * tap): order an image's rays by 16 x 16 tiles.
 * dr_project_bundle_bwd_rays writes d_origins and d_dirs [N][3] f32 (overwritten), as dr_march_bundle_bwd_rays does: the frozen
 * branches are n, the jitter draw, the slab faces, the t_near clamp, the cells and the argmax. t_near, jitter_seed and ray_base
 * must be those of the dr_bundle_setup call that made the buffers. A ray with n <= 1 gets zeros; D5 as above.
 * Invalid arguments (null required pointers, N <= 0, N >= 2^31, a volume extent < 2, max_samples < 1, a NaN t_near, an unknown
 * mode, variant or dtype, DR_PROJ_MAX without arg_max) return DR_EINVAL before any HIP call; a library linked without these
 * kernels returns DR_EUNSUPPORTED. */
int dr_project_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                          int64_t sx, int64_t sy, int64_t sz,
                          const float *origins, const float *dirs, const float *entry, const float *exit_,
                          const int32_t *nsamp, int64_t N, int max_samples, int mode,
                          float *out, int32_t *arg_max, void *stream);
int dr_project_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                          int64_t sx, int64_t sy, int64_t sz,
                          const float *origins, const float *dirs, const float *entry, const float *exit_,
                          const int32_t *nsamp, int64_t N, int max_samples, int mode,
                          const float *grad_out, const int32_t *arg_max,
                          float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int variant, void *stream);
int dr_project_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                               int64_t sx, int64_t sy, int64_t sz,
                               const float *origins, const float *dirs, const float *entry, const float *exit_,
                               const int32_t *nsamp, int64_t N, int max_samples, int mode,
                               float t_near, uint32_t jitter_seed, uint32_t ray_base,
                               const float *grad_out, const int32_t *arg_max,
                               float *d_origins, float *d_dirs, void *stream);

/* The differentiable march through a pre-classified RGBA volume over an arbitrary bundle of rays:
 * dr_march_rgba_fwd's DR_MODE_DIFF march and its backwards with a ray as an input, as dr_march_bundle_fwd / _bwd / _bwd_rays
 * are dr_march_fwd's. origins, dirs [N][3] f32 (UNIT directions, used as given), the ray buffers of dr_bundle_setup and N as
 * above; the volume's arguments are dr_march_rgba_fwd's (element strides sx, sy, sz and the channel stride sc; one volume per
 * call, no view stride; sc == 1 with every other stride a multiple of 4 and a 16-B (f32) / 8-B (f16) aligned pointer fetches a
 * voxel with one load, same bits). No table, no light, no shading.
 * dr_march_rgba_bundle_fwd: out_rgba [N][4] and steps [N] (nullable) as dr_march_rgba_fwd: the rays of a dr_ray_setup view with
 * its camera repeated as the origins give that view's image and steps bit for bit.
 * dr_march_rgba_bundle_bwd ACCUMULATES d_vol (f32; element strides dsx, dsy, dsz and channel stride dsc; caller zeroes); d_vol
 * NULL returns 0 before any HIP call. NaN propagates as in the plain kernels.
 * dr_march_rgba_bundle_bwd_rays writes d_origins and d_dirs [N][3] f32 (overwritten), as dr_march_bundle_bwd_rays does: the
 * frozen branches are those of dr_march_rgba_bwd_cam (n, `steps` of dr_march_rgba_bundle_fwd, the jitter draw, the slab faces,
 * the cells) and the t_near clamp. t_near, jitter_seed and ray_base must be those of the dr_bundle_setup call that made the
 * buffers. A ray with n <= 1 gets zeros; a NaN ray gets zeros and infinities are clamped to +-1e30 (D5).
 * Invalid arguments (null required pointers, N <= 0, N >= 2^31, a volume extent < 2, max_samples < 1, a NaN t_near, an unknown
 * dtype, a non-finite or non-positive sampling rate) return DR_EINVAL before any HIP call; a library linked without these
 * kernels returns DR_EUNSUPPORTED. */
int dr_march_rgba_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                             int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                             const float *origins, const float *dirs, const float *entry, const float *exit_,
                             const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                             float *out_rgba, int32_t *steps, void *stream);
int dr_march_rgba_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                             int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                             const float *origins, const float *dirs, const float *entry, const float *exit_,
                             const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                             const float *grad_out, const float *out_rgba,
                             float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, int64_t dsc, void *stream);
int dr_march_rgba_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                                  int64_t sx, int64_t sy, int64_t sz, int64_t sc,
                                  const float *origins, const float *dirs, const float *entry, const float *exit_,
                                  const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                                  const int32_t *steps, float t_near, uint32_t jitter_seed, uint32_t ray_base,
                                  const float *grad_out, const float *out_rgba,
                                  float *d_origins, float *d_dirs, void *stream);

/* Ray-depth moments of the differentiable 1-D TF march over an arbitrary bundle of rays: dr_march_depth_fwd and
 * its backwards with a ray as an input, as dr_march_bundle_fwd / _bwd / _bwd_rays are dr_march_fwd's, and with exactly their
 * argument lists. origins, dirs [N][3] f32 (UNIT directions, used as given), the ray buffers of dr_bundle_setup, N, the volume
 * (f32 or f16, any element strides) and the table [R][4] as above; one volume and one table per call. No light, no shading: only
 * the table's alpha column is read. All arithmetic is float32.
 * dr_march_depth_bundle_fwd: out_rgba [N][4] holds the moments (M1, M2, 0, A) = (sum w_s t_s, sum w_s t_s^2, 0, sum w_s),
 * w_s = T_s op_s, where t_s is the march's own parameter mix(t0, exit, s / (n - 1)): the distance of sample s from the ray's origin
 * along its unit direction. steps [N] is nullable. The rays of a dr_ray_setup view with its camera repeated as the origins give
 * dr_march_depth_fwd's moments and steps bit for bit; on any bundle A and steps are dr_march_bundle_fwd's alpha channel and steps.
 * With t_near = -INFINITY an origin inside the box collects negative distances behind it; t_near = 0 makes M1 / A a range.
 * dr_march_depth_bundle_bwd ACCUMULATES d_vol (element strides dsx, dsy, dsz) and the ALPHA column of d_tf [R][4] (caller zeroes;
 * the colour columns are never written); either may be NULL, both NULL returns 0 before any HIP call. grad_out [N][4]: its third
 * channel is never read. NaN propagates as in the plain kernels.
 * dr_march_depth_bundle_bwd_rays writes d_origins and d_dirs [N][3] f32 (overwritten), as dr_march_bundle_bwd_rays does: the
 * derivative w.r.t. the origin and w.r.t. the direction as a free 3-vector WITH t_s THE MARCH PARAMETER -- not the dot product
 * (pos - origin).dir, which for a free direction is t_s |dir|^2 and carries an extra radial term; through a caller that
 * normalises the directions the two agree. The frozen branches are those of dr_march_depth_bwd_cam (n, `steps` of
 * dr_march_depth_bundle_fwd, the jitter draw, the slab faces, the cells, 0 < x_tf) and the t_near clamp. t_near, jitter_seed and
 * ray_base must be those of the dr_bundle_setup call that made the buffers. A ray with n <= 1 gets zeros; a NaN ray gets zeros
 * and infinities are clamped to +-1e30 (D5).
 * Invalid arguments (null required pointers, N <= 0, N >= 2^31, a volume extent < 2, R < 1, max_samples < 1, a NaN t_near, an
 * unknown dtype, a non-finite or non-positive sampling rate) return DR_EINVAL before any HIP call; a library linked without
 * these kernels returns DR_EUNSUPPORTED. */
int dr_march_depth_bundle_fwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                              int64_t sx, int64_t sy, int64_t sz, const float *tf, int R,
                              const float *origins, const float *dirs, const float *entry, const float *exit_,
                              const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                              float *out_rgba, int32_t *steps, void *stream);
int dr_march_depth_bundle_bwd(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                              int64_t sx, int64_t sy, int64_t sz, const float *tf, int R,
                              const float *origins, const float *dirs, const float *entry, const float *exit_,
                              const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                              const float *grad_out, const float *out_rgba,
                              float *d_vol, int64_t dsx, int64_t dsy, int64_t dsz, float *d_tf, void *stream);
int dr_march_depth_bundle_bwd_rays(const void *vol, int vol_dtype, int VX, int VY, int VZ,
                                   int64_t sx, int64_t sy, int64_t sz, const float *tf, int R,
                                   const float *origins, const float *dirs, const float *entry, const float *exit_,
                                   const int32_t *nsamp, int64_t N, int max_samples, float sampling_rate,
                                   const int32_t *steps, float t_near, uint32_t jitter_seed, uint32_t ray_base,
                                   const float *grad_out, const float *out_rgba,
                                   float *d_origins, float *d_dirs, void *stream);

/* Momentum gradient step on the transfer function, in place (apply_grad, EX.py:375-381):
 *   momentum = gamma*momentum + lr*clamp(d_tf, -max_grad, max_grad);  tf = max(tf - momentum, 0)
 *   tf, d_tf, momentum [n] f32 (n = R*4). */
int dr_tf_momentum_step(float *tf, const float *d_tf, float *momentum, int n, float lr, float gamma,
                        float max_grad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFERENDER_HIP_H */
