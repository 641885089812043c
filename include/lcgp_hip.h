/* lcgp_hip.h -- C ABI of liblcgp_hip.so: the MI355X (gfx950) hot path of LCGP.
 *
 * The reference (mosesyhc/LCGP) is pure Python on TensorFlow; it has no FFI.  The "interface" each
 * entry point below replaces is therefore a span of reference Python (file:line cited per function).
 * The Python host side (lcgp_amd/lcgp.py) binds these with ctypes; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer on the current device unless marked "host";
 *  - matrices are row-major;  `dtype`: 0 = float64, 1 = float32 (the reference is float64 only);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call only ENQUEUES
 *    work on that stream and returns; no device memory is allocated, freed or synchronised inside
 *    and no other stream or event is created;
 *  - the library keeps NO mutable state (the only static is the thread-local text behind
 *    lcgp_last_error): schedule parameters travel with the call (lcgp_sched), so calls on different
 *    streams / devices / host threads are independent;
 *  - the caller owns all memory, including `workspace` (size from lcgp_workspace_bytes);  the content of `workspace` and
 *    of the `scratch` of lcgp_predict / lcgp_predict_grad on entry is irrelevant: every value a call reads there was
 *    written earlier in the same call or by the calls it documents as its input (lcgp_potrf_logdet -> lcgp_trtri ->
 *    lcgp_lauum, lcgp_nll_grad -> lcgp_predict); tests/test_gpu_stage_bounds.py checks bitwise-equal results on zero,
 *    NaN and 0x5A-filled memory;
 *  - return value 0 = enqueued; < 0 = bad argument / HIP error (see lcgp_last_error()).
 *    A non positive-definite matrix is reported through the `info` word of the output block,
 *    not through the return value (the call is asynchronous).
 *
 * theta block (host computes it, one H2D copy per evaluation), per local component k, doubles:
 *     [ ell_0 .. ell_{d-1} | scale | nug | D_k | psi_0 .. psi_{p-1} ]        width d + 3 + p
 *   ell/scale/nug are the CONSTRAINED values (what the reference calls lLmb[k], lLmb0[k],
 *   lnugGPs[k]; lcgp.py:515-532), D_k = diag_D[k] (lcgp.py:480), psi = phi[:,k]/sigma
 *   (lcgp.py:646) -- for the replicated path sigma is sigma_used (lcgp.py:576-584).
 *
 * output block, per local component k, doubles:
 *     [ half_logdet | quad | info | g_ell_0 .. g_ell_{d-1} | g_scale | g_nug | gsig_0 .. gsig_{p-1} ]
 *                                                                         width d + 5 + p
 *   half_logdet = sum_i log L_ii            (= 1/2 log det A_k, A_k = I + D_k (C_k o s s^T))
 *   quad        = b^T (b - A_k^-1 b)        (so NLL_k = half_logdet - quad / (2 D_k))
 *   info        = 0, or 1 + index of the first non-positive pivot
 *   g_*         = d NLL_k / d (constrained ell, scale, nug)
 *   gsig_a      = sum_i Y[a,i] (b_i - z_i)  (host turns it into d NLL / d lsigma2s)
 */
#ifndef LCGP_HIP_H
#define LCGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCGP_F64 0
#define LCGP_F32 1

/* `kernel_id`: the covariance kernel of the latent components.
 *   LCGP_KERNEL_MATERN32  the reference's kernel (covmat.py:31-55): C0 = prod_j (1 + S_j) exp(-sum_j S_j), S_j = |dx_j| / ell_j
 *   LCGP_KERNEL_SE        squared-exponential product kernel, C0 = exp(-1/2 sum_j S_j^2).  The reference has NO such kernel
 *                         (covmat.py holds Matern32 only); BASELINE.json's north star names it, so the path carries it as an
 *                         extension with the same nugget / scale structure.  Parity for it is UNPINNED: it is checked against
 *                         this repository's own oracle through identities only (gradient = finite differences = autograd,
 *                         eigendecomposition form = Cholesky form), never against the reference.
 *   LCGP_KERNEL_MATERN52  Matern-5/2 product kernel in the convention of LCGP_KERNEL_MATERN32 (no sqrt(5) factor):
 *                         C0 = prod_j (1 + S_j + S_j^2 / 3) exp(-sum_j S_j), which is the textbook Matern-5/2 at lengthscale
 *                         sqrt(5) ell_j per dimension.  Twice differentiable sample paths (Matern-3/2: once; the PREDICTIONS of all three
 *                         kernels have the input Hessians of lcgp_predict_hess).  The reference
 *                         has no such kernel either: an extension like LCGP_KERNEL_SE, parity UNPINNED, tied to identities
 *                         only.  Every call that takes a kernel_id accepts it. */
#define LCGP_KERNEL_MATERN32 0
#define LCGP_KERNEL_SE 1
#define LCGP_KERNEL_MATERN52 2

/* library version (major*100 + minor), hash of the sources the binary was built from
 * (sha256 of lcgp_hip.hip + lcgp_hip.h, first 16 hex digits; "unknown" if built without
 * -DLCGP_SRC_HASH) and the last error text of the calling thread (host strings). */
int lcgp_version(void);
const char* lcgp_source_hash(void);
const char* lcgp_last_error(void);

/* width of the theta / output blocks described above, and of the reduced vector of lcgp_pack_partial. */
int lcgp_theta_width(int d, int p);
int lcgp_out_width(int d, int p);
int lcgp_partial_width(int d, int p, int q_total);

/* Schedule of the factorisation / inverse (launch shapes only: results do not depend on it beyond
 * rounding).  Passed per call as the last argument of the entry points that schedule launches;
 * NULL = the defaults lcgp_sched_default() writes.  All counts are 64x64 or 128x128 tile counts
 * TIMES the number of local components. */
typedef struct lcgp_sched {
    int outer_blocks;       /* width of the outer Cholesky panel in 64-column blocks; 0 = automatic (4 fp64, 8 fp32) */
    int syrk_small_tiles;   /* a trailing update with fewer 128x128 tiles than this runs on 64x64 tiles (3000) */
    int trtri_small_tiles;  /* the whole triangular inverse runs on 64x64 tiles below this many 128x128 tiles (4200) */
    int lauum_small_tiles;  /* the same for A^-1 = W^T W (2048) */
    int trtri_level_small;  /* a single level of the triangular inverse below this many 128x128 tiles: 64x64 tiles (600) */
    int fill_leaf;          /* filler blocks (128x64 tiles of the previous panel's trailing update) carried by a
                               diagonal-block launch (248 = one per otherwise idle CU; 0 = none) */
    int fill_step;          /* filler blocks carried by a chain-step launch that ends in a diagonal block (248) */
    int leaf_in_wide;       /* a trailing update of at most this many 64x64 tiles also factors the next panel's first
                               diagonal block, so that panel's chain starts one launch earlier (2048; 0 = never) */
    int progressive_tiles;  /* lcgp_nll_grad only: with at most this many 128x128 lower tiles x components (few components
                               per rank) L^-1 and A^-1 are formed panel by panel BEHIND the factorisation, as filler tiles
                               of the chain launches, instead of after it (600; 0 = never) */
    int progressive_far;    /* with the progressive inverse: 1 = the far columns of a trailing update still ride on the next
                               panel's chain launches, 0 = every trailing update is one wide launch (the chain launches
                               carry the jobs of the inverse only) */
    int progressive_lauum;  /* with the progressive inverse: A^-1 = W^T W is accumulated behind the chain as well when the matrix
                               has at most this many 64-blocks per side (48); beyond, only L^-1 is, and A^-1 takes the one
                               launch of lcgp_lauum after the factorisation (0 = always that) */
    int pair_tiles;         /* two consecutive panels share ONE trailing update with K = 2 panels on the columns between the
                               second panel and the far columns when that region holds at least this many 64x64 tiles (the
                               first panel then only updates the second panel's own columns) (4000; 0 = never) */
} lcgp_sched;
int lcgp_sched_default(lcgp_sched* sched /*host out*/);

/* bytes of `workspace` needed by lcgp_nll_grad / lcgp_potrf_logdet / lcgp_potri for q_local components,
 * and of the `scratch` of lcgp_predict for n0 new inputs. */
int lcgp_workspace_bytes(int dtype, int n, int d, int p, int q_local, size_t* bytes /*host out*/);
int lcgp_predict_scratch_bytes(int dtype, int n, int q_local, int n0, size_t* bytes /*host out*/);

/* Matern32(x1, x2, llmb, llmb0, lnug)  -- covmat.py:5-55 (build branch 31-55).
 * out (n1 x n2, row-major).  `same` != 0 adds the nugget term on the diagonal (the reference adds it
 * iff x1 and x2 have equal shape and bitwise-equal values, covmat.py:46-51; the caller decides). */
int lcgp_matern32(void* stream, int dtype, int n1, int n2, int d,
                  const void* x1, const void* x2,
                  const double* ell /*host, d*/, double scale, double nug, int same, void* out);
/* the same for any kernel_id (lcgp_matern32 = lcgp_covmat with LCGP_KERNEL_MATERN32) */
int lcgp_covmat(void* stream, int dtype, int kernel_id, int n1, int n2, int d,
                const void* x1, const void* x2,
                const double* ell /*host, d*/, double scale, double nug, int same, void* out);

/* K1: A_k = I + D_k * (C_k o sr sr^T) for all local components, into the workspace
 * (lcgp.py:651 for the full path; lcgp.py:606 + 616 for the replicated path, sr = sqrt(r)).
 * Only the lower-triangular 64x64 tiles are written.  sr may be NULL (all ones). */
int lcgp_kernel_build(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                      const void* x /*n x d*/, const void* sr /*n or NULL*/,
                      const double* theta, void* workspace);

/* K2: blocked Cholesky A_k = L_k L_k^T of the matrices left by lcgp_kernel_build, in place, plus
 * the inverses of the 64x64 diagonal blocks needed later.  Replaces tf.linalg.eigh (lcgp.py:652) /
 * tf.linalg.cholesky (lcgp.py:617) and the log-determinant (lcgp.py:660 / 624).
 * half_logdet (q_local doubles) and info (q_local ints) are written on the device (either may be NULL). */
int lcgp_potrf_logdet(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace,
                      double* half_logdet, int* info, const lcgp_sched* sched /*host or NULL*/,
                      const void* plan /*host, or NULL*/);

/* K4: A_k^-1 (lower tiles) from the factor left by lcgp_potrf_logdet.  Replaces the dense
 * U diag(.) U^T products of lcgp.py:654 / 705-715 and cholesky_solve with identity (lcgp.py:785). */
int lcgp_potri(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace,
               const lcgp_sched* sched);

/* the two stages of lcgp_potri on their own (for per-kernel timing): W = L^-1 (level-parallel triangular
 * products), then A^-1 = W^T W (a single launch of the MFMA tile kernel; n^3/3 flops per component). */
int lcgp_trtri(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace, const lcgp_sched* sched);
int lcgp_lauum(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace, const lcgp_sched* sched);

/* Measurement support (no counterpart in the reference): wave 0 of the first workgroup of
 *   - the launch that forms A^-1 = W^T W (lcgp_lauum, and the same launch inside lcgp_nll_grad), in either tile size, and
 *   - the first (widest) trailing update of every factorisation -- which is what remains to be stamped in the configurations
 *     whose A^-1 is accumulated behind the factorisation (few components per rank, small n: lcgp_sched.progressive_*)
 * stamps its K loop with the shader-clock counter and with the 100 MHz real-time counter; this copies the two durations of
 * the LAST stamped launch to `out` (device, 2 x 64 bit: shader cycles, 10 ns ticks) and CLEARS them: zeros mean that no
 * stamped launch has run since the last call (a fresh workspace holds garbage until the first call).
 * cycles / ticks x 100 = the clock in MHz the chip held while the fp64 MFMA pipe was loaded, measured in the un-profiled
 * path (bench.py: roofline.clock_mhz).  The window is approximate -- the stamps are scalar instructions the compiler may
 * move a few instructions into the tile's prologue / epilogue -- and short in small configurations (tens of microseconds:
 * the ratio then carries the 10 ns granularity of the real-time counter, ~0.1 %). */
int lcgp_lauum_clock(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace,
                     unsigned long long* out /*device, 2 words*/);

/* copies matrix `which` (0 = A/L, 1 = L^-1, 2 = A^-1) of local component k out of the workspace as a
 * dense n x n row-major matrix (lower triangle valid, upper triangle mirrored); for tests. */
int lcgp_fetch_matrix(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace,
                      int which, int k, void* out /*n x n*/);

/* copies vector `which` (0 = b_k, 1 = z_k = A_k^-1 b_k) of local component k (n elements of dtype). */
int lcgp_fetch_vector(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace,
                      int which, int k, void* out /*n*/);

/* The whole hot path for q_local components: build + Cholesky + inverse + z = A^-1 b + fused gradient
 * contraction.  Replaces one call of LCGP.neglpost (lcgp.py:635-666) or LCGP.neglpost_rep
 * (lcgp.py:554-630) TOGETHER WITH the tf.GradientTape backward pass gpflow runs around it
 * (lcgp.py:538-539), for the components held by this rank.
 *   x  : n x d standardised inputs (x_unique_s for the replicated path)
 *   Y  : p x n outputs the latent targets are projected from (standardised y; sqrt(r) o ybar for rep)
 *   sr : NULL for the full path; sqrt(r) (n) for the replicated path
 *   theta, out : device blocks described at the top (q_local rows each) */
int lcgp_nll_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                  const void* x, const void* Y, const void* sr,
                  const double* theta, void* workspace, double* out, const lcgp_sched* sched,
                  const void* plan /*host, or NULL*/);

/* Exact Hessian of the objective in the parameters (the reference would nest two gradient tapes around neglpost, lcgp.py:635-666
 * / 554-630; this entry replaces them).  float64 only: LCGP_F32 is refused with an error text (the kernel block is the
 * difference of two traces that cancel heavily, and the call is made once per fit).
 * Runs behind lcgp_nll_grad at the same theta and only READS its workspace (A_k^-1 lower tiles, b_k, z_k): lcgp_predict and the
 * other post-fit entries stay valid after it.  Per local component k, with A = I + D (C o s s^T), C = scale ((1 - w) C0 + w I),
 * w = nug / (1 + nug), z = A^-1 b, b = sum_a psi_a Y_a, c_a = psi_a Y_a, the component's share of the objective is
 * f_k = 1/2 log det A - b^T (b - z) / (2 D), and for the m = d + 2 kernel parameters theta_i in [ell_0 .. ell_{d-1}, scale, nug],
 * G_i = A^-1 d_iA, y_i = d_iA z, and the built noise parameters t_a (psi_a = phi_ak / sig_a, sig_a = exp(t_a / 2) / std_a):
 *     hk[i, j] = 1/2 sum (A^-1 o d_ijA) - 1/2 tr(G_i G_j) - z^T d_ijA z / (2 D) + y_i^T A^-1 y_j / D          (m x m, symmetric)
 *     hx[i, a] = c_a^T A^-1 y_i / (2 D)                                                                       (m x p)
 *     hn[a, b] = -[ delta_ab c_a^T (b - z) + c_a^T (I - A^-1) c_b ] / (4 D)                                   (p x p)
 *   kernel derivatives in ell with S_i = |dx_i| / ell_i: d_i C0 = C0 phi_i, d_ij C0 = C0 (phi_i phi_j + delta_ij d phi_i / d ell_i),
 *       Matern-3/2: phi = S^2 / ((1 + S) ell)      SE: phi = S^2 / ell      Matern-5/2: phi = S^2 (1 + S) / (ell (3 + 3 S + S^2))
 *   d_scale A and d_nug A are combinations of A, I and diag(s^2): G_scale, G_nug, y_scale, y_nug need no matrix product.
 * Output: row k of `out` (q_local rows of lcgp_nll_hess_width(d, p) = m^2 + m p + p^2 doubles) = [ hk | hx | hn ], row-major
 * blocks.  The caller sums hn over the components, adds the term of the objective outside the components
 * (delta_ab ysq_a / (2 sig_a^2)), folds both noise blocks through the error-structure groups and applies the 1 / n of the
 * replicated path.  Kernel blocks of different components are exactly zero and are not written.
 * The call handles the components k0 .. k0 + q_group - 1 of the workspace (carved for q_local) and writes their rows of
 * `out`: a caller bounds the scratch by processing the local components in groups.  Launches: A^-1 mirrored to a full matrix
 * with G_scale / G_nug beside it; per dimension i one launch that materialises d_iA (one buffer, reused: the tile kernel then
 * stages plain dense operands, and the same buffer gives y_i = d_iA z), and G_i = A^-1 d_iA on the fp64 MFMA tile kernel
 * (operand mode OP_HESS_G, 128 x 128 tiles); the pairwise traces tr(G_i G_j) by a tile-transposing reduction; a second-order
 * fused contraction that recomputes C0, phi_i and d phi_i / d ell_i in registers (no n x n x d x d tensor is written);
 * u_i = A^-1 y_i; Q = Y A^-1 on the tile kernel; the dot products of the three blocks.
 * scratch: lcgp_nll_hess_scratch_bytes(dtype, n, d, p, q_group) bytes = q_group (d + 4) npad^2 doubles (A^-1, d_iA, the d + 2
 *   G_i) plus q_group (3 d + 4 + ppad) npad and ppad npad doubles of vectors, Q and the padded Y (ppad = p rounded up to 128) and
 *   the per-band partial sums; its content on entry is irrelevant.
 * Flops per component: 2 d npad^3 (the products G_i) + 2 ppad npad^2 (Q) + (d + 2)(d + 3) npad^2 (the traces); every sum has a
 * fixed order, no atomics: bitwise reproducible, independent of q_local, of q_group and of the scratch content on entry. */
int lcgp_nll_hess_width(int d, int p);
int lcgp_nll_hess_scratch_bytes(int dtype, int n, int d, int p, int q_group, size_t* bytes /*host out*/);
int lcgp_nll_hess(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                  const void* x, const void* Y, const void* sr, const double* theta, const void* workspace,
                  int k0, int q_group, void* scratch, double* out /*q_local rows of lcgp_nll_hess_width(d, p)*/);

/* Parameter derivatives of the prediction (the reference gets them by a tf.GradientTape around predict, lcgp.py:808-930, over
 * the trainable variables; this entry replaces that tape).  float64 only: LCGP_F32 is refused with an error text (the variance
 * derivatives are differences that cancel).  Runs behind lcgp_nll_grad at the same theta and only READS its workspace (L_k^-1,
 * b_k, z_k): every other post-fit entry stays valid after it.  Per local component k, in the notation of lcgp_nll_hess, with
 * X_i the cross-covariance row of lcgp_predict for new input i (standardised; `same` as there: the row's nugget entry),
 * V_i = X_i A^-1, ghat_i = X_i . z, gvar_i = scale - D X_i . V_i, y_t = d_tA z and t in [ell_0 .. ell_{d-1}, scale, nug]:
 *     dghat[k, i, t]       = (d_t X_i) . z - V_i . y_t
 *     dgvar[k, i, t]       = d_t scale - D [ 2 (d_t X_i) . V_i - V_i (d_tA) V_i^T ]
 *     dghat_noise[k, i, a] = -1/2 psi_a V_i . Y_a          (the built noise parameters t_a of lcgp_nll_hess; d gvar / d t_a = 0)
 *   d_ell_j X_i = Xc_i o phi_j(x0_i, .) with Xc the continuous part of the row (phi_j = 0 at the nugget entry) and the phi of
 *   lcgp_nll_hess; d_scale X_i = X_i / scale; d_nug X_i = -Xc_i / (1 + nug) + scale s e_c* / (1 + nug)^2 at the nugget entry c*.
 *   d_scale A = (A - I) / scale and d_nug A = [D scale diag(s^2) - (A - I)] / (1 + nug) need no product: V_i A = X_i, so
 *   V_i (A - I) V_i^T = X_i . V_i - |V_i|^2.  Only the d terms V_i (d_jA) V_i^T do.
 * The call handles the components k0 .. k0 + q_group - 1 of the workspace (carved for q_local) and writes their rows of the
 * outputs: a caller bounds the scratch by processing the local components in groups and the new inputs in chunks.
 * Launches: x / ell, y_scale, y_nug (the first launch of lcgp_nll_hess); X, U = X W^T, ghat / gvar and V = U W by the launches
 * of lcgp_predict_grad (ghat / gvar are BITWISE those of lcgp_predict with the same `same`; V overwrites X); per dimension j:
 * d_jA materialised into one reused buffer, y_j = d_jA z, T_j = V d_jA on the fp64 MFMA tile kernel (operand mode OP_HESS_G, 128 x
 * 128 tiles, over U) and one wave per new input for T_j[i, :] . V_i; a fused row kernel, one workgroup per (new input, block of 16
 * dimensions), that recomputes C0 and phi_j in registers and accumulates every remaining sum in one sweep over the row (no n0 x n
 * x d tensor is written); V Y^T on the tile kernel (Y^T zero padded); one combining launch.
 * Outputs: ghat / gvar q_local rows of n0, `out_stride` apart (0 = n0); dghat / dgvar [q_local][out_stride][d + 2];
 *   dghat_noise [q_local][out_stride][p] (a caller that works in chunks passes the chunk's offset and the total as stride).
 * scratch: lcgp_predict_paramgrad_scratch_bytes(dtype, n, d, p, q_group, n0) bytes = q_group (2 n0pad npad + npad^2) doubles (X / V,
 *   U / T_j, d_jA; n0pad = n0 rounded up to 128) plus q_group ((2 d + 2) npad + n0pad (ppad + 4 d + 8)) and npad ppad doubles of
 *   vectors, V Y^T, the sums and the padded Y^T (ppad = p rounded up to 128); its content on entry is irrelevant.  n0 <= 65535.
 * Flops per component: 2 d n0pad npad^2 (the products T_j) + n0pad npad^2 (U, V) + 2 n0pad ppad npad (V Y^T) + d npad^2 (d + 30)-ish
 * (d_jA) + n0 n (d + 40) ceil(d / 16)-ish in the row kernel; every sum has a fixed order, no atomics: bitwise reproducible,
 * independent of q_local, of q_group and of the scratch content on entry. */
int lcgp_predict_paramgrad_scratch_bytes(int dtype, int n, int d, int p, int q_group, int n0, size_t* bytes /*host out*/);
int lcgp_predict_paramgrad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                           const void* x, const void* Y, const void* sr, const double* theta, const void* workspace,
                           int k0, int q_group, int n0, const void* x0, int same, void* scratch,
                           double* ghat, double* gvar,            /* q_local rows of n0, `out_stride` apart */
                           double* dghat, double* dgvar,          /* [q_local][out_stride][d + 2] */
                           double* dghat_noise,                   /* [q_local][out_stride][p] */
                           int out_stride);

/* The launch plan of the factorisation, computed ONCE by the caller instead of in every evaluation (it depends on
 * dtype, n, q_local, the schedule and on whether the inverse follows -- with_inverse = 1 for lcgp_nll_grad, 0 for
 * lcgp_potrf_logdet -- and on nothing else).  The plan is a position-independent block of `bytes` bytes in HOST memory
 * owned by the caller, passed to lcgp_nll_grad / lcgp_potrf_logdet, whose `sched` argument is then ignored (the plan
 * carries the schedule it was built for).  plan = NULL: the plan is computed per call.  The library still keeps no
 * state.  Replaces nothing in the reference: it is the cost of ~120 kernel launches the reference never had.
 * lcgp_plan_info: number of launches, and what the plan leaves behind the factorisation (0 = L, 1 = and L^-1,
 * 2 = and A^-1). */
int lcgp_plan_bytes(int dtype, int n, int q_local, int with_inverse, const lcgp_sched* sched, size_t* bytes /*host out*/);
int lcgp_plan_build(int dtype, int n, int q_local, int with_inverse, const lcgp_sched* sched,
                    void* plan /*host out*/, size_t bytes);
int lcgp_plan_info(const void* plan /*host*/, int* nlaunch, int* inverse_done);

/* Assembles this rank's share of the vector the ranks all-reduce (in the reference the sum over
 * k of lcgp.py:650-661 and the gradient tape's accumulation), on the device, in a fixed summation order:
 *   vec = [ sum_k (half_logdet_k - quad_k/(2 D_k)) | sum_k info_k | g_ell (q_total x d) | g_scale (q_total) |
 *           g_nug (q_total) | g_sigma (p) | guard ]                  width lcgp_partial_width(d, p, q_total)
 * with g_sigma_a = sum_k psi_k[a] gsig_k[a] / (2 D_k) over the LOCAL components; the slots of component i of
 * this rank are written at its global index comp[i] (device ints), all other slots are zeroed.  q_local may
 * be 0 (a rank without components contributes zeros).  `guard` (device, one double, or NULL = 0) is copied into the
 * last slot: the caller puts a hash of the parameter vector it evaluated there and compares the all-reduced value
 * with world_size x its own -- ranks running the optimiser in lock-step detect a drift at the first evaluation. */
int lcgp_pack_partial(void* stream, int d, int p, int q_local, int q_total, const int* comp,
                      const double* theta, const double* out, const double* guard, double* vec);

/* K6 prediction (lcgp.py:808-859 / 864-930 with the caches of 685-803): for local component k and
 * n0 new inputs x0 (already standardised) computes
 *     ghat[k, :] = c0k (sr o z_k)                       (lcgp.py:831 / 888)
 *     gvar[k, :] = scale_k - D_k rowsum((c0k o sr) A_k^-1 (c0k o sr)^T)   (lcgp.py:832 / 891-894)
 * using L_k^-1 and z_k left in the workspace by the last lcgp_nll_grad call with the same theta.
 * `same`: 0 = x0 is not the training set; s >= 1 = row i of x0 IS training input i + s - 1 (x0 is the training set or a
 * contiguous chunk of it starting at row s - 1), so the nugget term goes to that entry (covmat.py:46-51).
 * scratch: lcgp_predict_scratch_bytes(dtype, n, q_local, n0) bytes.
 * out_stride: elements between the rows of ghat / gvar (0 = n0): a caller that predicts a long batch in chunks passes
 * the chunk's offset into its (q_local x total) arrays and the total as stride, so no per-chunk temporaries are needed. */
int lcgp_predict(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                 const void* x, const void* sr, const double* theta, const void* workspace,
                 int n0, const void* x0, int same, void* scratch,
                 double* ghat /*q_local rows of n0*/, double* gvar /*q_local rows of n0*/, int out_stride);

/* Box-averaged predictions (no counterpart in the reference): the posterior mean and variance of latent component k AVERAGED
 * over a subset of the inputs, uniform on the box [lo_l, hi_l] (standardised inputs, hi_l > lo_l).  Row i of x0 carries a mask
 * (mask[i d + l] != 0: dimension l is integrated out; the entry x0[i, l] is then never read, a NaN there does not matter).
 * For the three product kernels the average of the cross-covariance row is a product of 1-D integrals of the kernel factor
 * kappa(u), u = |t - x| / ell (F(b) = int_0^b kappa, G(b) = int_0^b u kappa(u) du, in closed form):
 *     I1[k, l, j] = (ell / w) [sgn(x_jl - lo) F(|x_jl - lo| / ell) + sgn(hi - x_jl) F(|hi - x_jl| / ell)]     (w = hi_l - lo_l)
 *     I2[k, l]    = 2 ell [w F(a) - ell G(a)] / w^2,   a = w / ell                                        (ell = ell_kl)
 *     Xbar_k[i, j] = scale_k (1 - nt_k) prod_{l not in mask_i} kappa(|x0_il - x_jl| / ell_kl) prod_{l in mask_i} I1[k, l, j] sr_j
 *     ghat[k, i] = Xbar_k[i, :] z_k          gvar[k, i] = prior_ki - D_k |Xbar_k[i, :] W_k^T|^2
 *     prior_ki = scale_k (1 - nt_k) prod_{l in mask_i} I2[k, l]  (ascending l; nt = nug / (1 + nug): the nugget is white noise
 *     whose average over a set of positive measure vanishes);  a row with an EMPTY mask has prior scale_k and is bitwise the
 *     row of lcgp_predict(..., same = 0, ...) when both are formed on the same tile size (n0 below 128 in both, or not).
 * Launches: one writes the table I1 (q_local d npad doubles) and I2 into the scratch, the rows are formed by the kernel of
 * lcgp_predict compiled with the mask and table as extra inputs, then U = Xbar W^T on the tile kernel and the row reductions
 * as in lcgp_predict.  Summation order fixed, no atomics: results are bitwise reproducible and independent of q_local, of the
 * scratch content on entry and, between calls that use the same tile size, of how a caller splits the rows.
 * mask: device, n0 x d bytes.  box: device, 2 d doubles, lo then hi.
 * scratch: lcgp_predict_marginal_scratch_bytes(dtype, n, d, q_local, n0) = lcgp_predict_scratch_bytes + 8 q_local d (npad + 1). */
int lcgp_predict_marginal_scratch_bytes(int dtype, int n, int d, int q_local, int n0, size_t* bytes /*host out*/);
int lcgp_predict_marginal(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                          const void* x, const void* sr, const double* theta, const void* workspace,
                          int n0, const void* x0, const unsigned char* mask, const double* box, void* scratch,
                          double* ghat /*q_local rows of n0*/, double* gvar /*q_local rows of n0*/, int out_stride);

/* Input gradients of the prediction (the reference gets them by a tf.GradientTape around predict, lcgp.py:808-930 with
 * covmat.py:31-55; this entry point replaces that tape).  All derivatives are with respect to the STANDARDISED inputs x0s;
 * output row i depends only on row i of x0, so the Jacobian is per point.  With X_k = c0k o sr^T, W_k = L_k^-1, U_k = X_k W_k^T,
 * z_k = A_k^-1 b_k exactly as in lcgp_predict, for local component k, new input i and dimension l:
 *     dghat[k, i, l] =        sum_j dc_l(i, j) sr_j z_k[j]
 *     dgvar[k, i, l] = -2 D_k sum_j dc_l(i, j) sr_j V_k[i, j],      V_k = X_k A_k^-1 = U_k W_k
 *     dc_l = -c0 dx_l / (ell_l^2 (1 + S_l))   (Matern-3/2; dx_l = x0_il - x_jl, S_l = |dx_l| / ell_l; 0 at dx_l = 0)
 *     dc_l = -c0 dx_l / ell_l^2               (squared exponential)
 *   c0 includes scale (1 - nug / (1 + nug)).  Nugget convention: the nugget term is a point mass the reference adds only when
 *   x0 IS the training set; it has no derivative, so this is the gradient of the continuous prediction surface: same = 0
 *   throughout, training inputs included.  ghat / gvar are written as well and are BITWISE those of
 *   lcgp_predict(..., same = 0, ...) (the same launches).
 * Input: the workspace of the last lcgp_nll_grad at the same theta, as for lcgp_predict.
 * scratch: lcgp_predict_grad_scratch_bytes(dtype, n, q_local, n0) bytes (= lcgp_predict_scratch_bytes); its content on entry
 *   is irrelevant.  V_k overwrites X_k in it once the row reductions have read X_k.
 * Outputs: ghat / gvar q_local rows of n0, `out_stride` apart (0 = n0); dghat / dgvar q_local x n0 x d, row k at
 *   k * out_stride * d (a caller that works in chunks passes the chunk's offset and the total as stride, as for lcgp_predict).
 * Flops per component: n0pad npad^2 / 2 (U, as lcgp_predict) + n0pad npad^2 / 2 (V; n0pad = n0 rounded up to 128, or 64 below
 * 128) + ~n0 n (12 d + 30) in the contraction, which never forms the n0 x n x d derivative tensor; the reduction order is fixed
 * (no atomics): bitwise reproducible and independent of q_local. */
int lcgp_predict_grad_scratch_bytes(int dtype, int n, int q_local, int n0, size_t* bytes /*host out*/);
int lcgp_predict_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                      const void* x, const void* sr, const double* theta, const void* workspace,
                      int n0, const void* x0, void* scratch,
                      double* ghat, double* gvar,        /* q_local rows of n0, `out_stride` apart */
                      double* dghat, double* dgvar,      /* q_local x n0 x d, row k at k * out_stride * d */
                      int out_stride);

/* Input Hessians of the prediction (the reference gets them by nesting two gradient tapes around predict; this entry point
 * replaces both).  Derivatives with respect to the STANDARDISED inputs, per point, same = 0 throughout as in lcgp_predict_grad.
 * With X_k, W_k, U_k, V_k, z_k as there, s_l = (x0_il - x_jl) / ell_l, a = |s_l|, for local component k, new input i and
 * dimensions l, m:
 *     d_l c     = c phi_l,  phi_l = -h(s_l) / ell_l      d2_lm c = c phi_l phi_m  (l != m)      d2_ll c = c psi(s_l) / ell_l^2
 *       Matern-3/2: h = s / (1 + a)                 psi = -(1 - a) / (1 + a)        (continuous at 0, with a kink there)
 *       SE        : h = s                           psi = s^2 - 1
 *       Matern-5/2: h = s (1 + a) / (3 + 3 a + a^2) psi = -(1 + a - a^2) / (3 + 3 a + a^2)
 *     d2ghat[k, i, l, m] =        sum_j d2_lm c(i, j) sr_j z_k[j]
 *     d2gvar[k, i, l, m] = -2 D_k (sum_j d2_lm c(i, j) sr_j V_k[i, j] + P_il . P_im),   P_il = (d_l X_i) W_k^T  (n elements)
 * ghat, gvar, dghat, dgvar are written as well and are BITWISE those of lcgp_predict_grad (the same launches, enqueued first).
 * Then: one launch writes the rows d_l X_i (row i d + l, without their factor -1 / ell_l, zero padded to whole tiles), the
 * tile kernel forms P (the product of lcgp_predict's U on n0 d rows), one wave per point and 4 x 4 block of dimension pairs
 * forms the dot products P_il . P_im, and a fused contraction (c recomputed in registers, V staged through LDS, the n0 x n x d x
 * d tensor never written) adds the sums over j and applies -2 D_k / (ell_l ell_m).
 * Input: the workspace of the last lcgp_nll_grad at the same theta, as for lcgp_predict.
 * scratch: lcgp_predict_hess_scratch_bytes(dtype, n, d, q_local, n0) bytes = 2 q_local (n0pad + rpad) npad elements, n0pad as in
 *   lcgp_predict, rpad = n0 d rounded up to 128 (to 64 below 128); its content on entry is irrelevant.
 *   n0 d <= LCGP_HESS_MAX_ROWS (a caller with more passes the new inputs in chunks, as for lcgp_predict).
 * Outputs: the four of lcgp_predict_grad; d2ghat / d2gvar q_local x n0 x d (d + 1) / 2, the packed lower triangle, entry
 *   (l, m <= l) at l (l + 1) / 2 + m, row k at k * out_stride * d (d + 1) / 2.
 * Flops per component: those of lcgp_predict_grad + rpad npad^2 / 2 (P) + 2 n0 n d (d + 1) / 2-ish in the dot products and the
 * contraction; the reduction order is fixed (no atomics): bitwise reproducible, independent of q_local, of how a caller splits
 * the new inputs over calls and of the scratch content on entry. */
#define LCGP_HESS_MAX_ROWS 4194304
int lcgp_predict_hess_scratch_bytes(int dtype, int n, int d, int q_local, int n0, size_t* bytes /*host out*/);
int lcgp_predict_hess(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                      const void* x, const void* sr, const double* theta, const void* workspace,
                      int n0, const void* x0, void* scratch,
                      double* ghat, double* gvar,        /* q_local rows of n0, `out_stride` apart */
                      double* dghat, double* dgvar,      /* q_local x n0 x d, row k at k * out_stride * d */
                      double* d2ghat, double* d2gvar,    /* q_local x n0 x d (d + 1) / 2, row k at k * out_stride * d (d + 1) / 2 */
                      int out_stride);

/* Posterior covariance of the latent GRADIENT at new inputs, and its weighted sum over them (no counterpart in the reference).
 * With X_k, W_k as above and the rows P_il of lcgp_predict_hess, for local component k, new input i (standardised) and
 * dimensions l, m: the posterior covariance function Sigma_k(x, x') = c_k(x, x') - D_k X_k(x) W_k^T W_k X_k(x')^T of the
 * continuous surface (no nugget term: a point mass has no derivative, as in lcgp_predict_grad) differentiated once in each
 * argument at x = x' = x0_i:
 *     Gamma[k, i, l, m] = delta_lm c_k kappa / ell_l^2 - D_k (P_il . P_im) / (ell_l ell_m)
 *     c_k = scale_k (1 - nug_k / (1 + nug_k)), the continuous part of the prior variance;  kappa = -f''(0) of the 1-D factor:
 *     1 (Matern-3/2), 1 (SE), 1 / 3 (Matern-5/2).  f'(0) = 0 for all three, so the prior part is diagonal.
 *     dghat[k, i, l] BITWISE that of lcgp_predict_grad (its contraction without the variance half; V_k is not formed).
 *     M[k, l, m]    += sum_i w_i Gamma[k, i, l, m]            when w is given
 * Launches: the mean half of lcgp_predict_grad's contraction, the rows d_l X_i and P as in lcgp_predict_hess, then one wave per
 * (new input, 4 x 4 block of dimension pairs) for the dot products and Gamma; with w, every workgroup leaves its weighted
 * sum in the scratch and a second launch adds them to M in index order (no atomics).
 * scratch: lcgp_predict_gradcov_scratch_bytes(dtype, n, d, q_local, n0) bytes = 2 q_local rpad npad elements, rpad = n0 d rounded
 *   up to 128 (to 64 below 128): less than lcgp_predict_hess_scratch_bytes.  n0 d <= LCGP_HESS_MAX_ROWS.
 * Outputs: dghat as in lcgp_predict_grad; gamma q_local x n0 x d (d + 1) / 2 packed as d2gvar is, or NULL with w given: the
 *   per-point tensor is then never written.  w: n0 doubles on the device or NULL.  M: q_local x d (d + 1) / 2, contiguous,
 *   ADDED to (a caller that passes the new inputs in chunks carries it across calls and zeroes it first); required with w.
 * dghat and gamma are bitwise reproducible, independent of q_local, of w, of the scratch content on entry and, between calls
 * that use the same tile size for P (rpad a multiple of 128 or not), of how a caller splits the new inputs; M is bitwise
 * reproducible for the same split and does not depend on whether gamma is written. */
int lcgp_predict_gradcov_scratch_bytes(int dtype, int n, int d, int q_local, int n0, size_t* bytes /*host out*/);
int lcgp_predict_gradcov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                         const void* x, const void* sr, const double* theta, const void* workspace,
                         int n0, const void* x0, void* scratch,
                         double* dghat,                  /* q_local x n0 x d, row k at k * out_stride * d */
                         double* gamma,                  /* q_local x n0 x d (d + 1) / 2, row k at k * out_stride * d (d + 1) / 2; or NULL */
                         const double* w,                /* n0 weights, or NULL */
                         double* M,                      /* q_local x d (d + 1) / 2, added to; NULL without w */
                         int out_stride);

/* Joint posterior covariance over new inputs, and correlated draws (no counterpart in the reference: its predict is marginal
 * only).  For local component k and n0 new inputs x0 (standardised), with c0k, sr, L_k^-1 exactly as in lcgp_predict:
 *     Sigma_k = C00_k - D_k U_k U_k^T,   U_k = (c0k o sr^T) L_k^-T    (n0 x n),   diag(Sigma_k) = gvar[k, :] of lcgp_predict
 *     C00_k   = the covariance kernel of x0 with itself, nugget on the diagonal (lcgp_covmat with same = 1)
 * The result is written into a SECOND workspace, `cov_workspace`, of lcgp_workspace_bytes(dtype, n0, d, p, q_local) bytes:
 * its matrix slot (lcgp_fetch_matrix(..., n0, ..., which = 0, k)) holds Sigma_k + tau_k I, tau_k = jitter * scale_k, lower
 * tiles valid, identity on the padding -- exactly what lcgp_potrf_logdet(dtype, n0, d, p, q_local, cov_workspace, ...)
 * factors in place (its info word reports a Sigma_k + tau_k I that is not numerically positive definite).
 *   `same`: as in lcgp_predict (the nugget term of the cross covariance c0k; 0 = x0 is not the training set).
 *   scratch: lcgp_predict_cov_scratch_bytes(dtype, n, q_local, n0) bytes.
 *   The content of `cov_workspace` and `scratch` on entry is irrelevant: the call writes every value it reads there
 *   (tests/test_gpu_joint_bounds.py runs it on memory filled three ways and compares bitwise).
 * Flops per component: n0pad^2 npad (the lower tiles of U U^T, n0pad = n0 rounded up to 128) + n0pad npad^2 / 2 (U). */
int lcgp_predict_cov_scratch_bytes(int dtype, int n, int q_local, int n0, size_t* bytes /*host out*/);
int lcgp_predict_cov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                     const void* x, const void* sr, const double* theta, const void* workspace,
                     int n0, const void* x0, int same, void* scratch, void* cov_workspace, double jitter);

/* Draws from the factor lcgp_potrf_logdet left in `cov_workspace` (L_k L_k^T = Sigma_k + tau_k I):
 *     out[k, s, :] = ghat[k, :] + L_k eps[k, s, :]          s < S
 * eps: q_local x S x n0 standard normals (dtype, dense); ghat: q_local rows of n0 doubles, `ldg` apart (0 = n0), e.g. the
 * ghat of lcgp_predict; out: q_local x S x n0 doubles.  The call zeroes the unused strict upper triangle of the factor's
 * diagonal tiles (the product reads whole tiles).  scratch: lcgp_sample_scratch_bytes(dtype, n0, q_local, S) bytes.
 * The content of `scratch` and `out` on entry is irrelevant; of `cov_workspace` only the factor in its matrix slot is read.
 * Flops per component: S n0pad^2 (S rounded up to 128). */
#define LCGP_SAMPLE_MAX 32768
int lcgp_sample_scratch_bytes(int dtype, int n0, int q_local, int S, size_t* bytes /*host out*/);
int lcgp_sample_latent(void* stream, int dtype, int n0, int d, int p, int q_local, int S, void* cov_workspace,
                       const void* eps, const double* ghat, int ldg, void* scratch, double* out);

/* Conditioning on new runs without refactorising (no counterpart in the reference; what BoTorch calls
 * condition_on_observations).  Input: the workspace of the last lcgp_nll_grad, which is only READ -- every other post-fit
 * entry stays valid.  For local component k, m new UNIQUE inputs xn (standardised, none of them a training input) with
 * replicate counts r_i and latent observations t_i, in the notation of lcgp_predict (W_k = L_k^-1):
 *     U_n  = (c(xn, x) o sr^T) W_k^T                      (m x npad; cross rows without nugget: lcgp_predict, same = 0)
 *     S    = C(xn, xn) - D_k U_n U_n^T + diag(tau),       C(xn, xn) with the nugget on its diagonal (lcgp_predict_cov's C00),
 *            tau_i = 1 / (D_k r_i)                        (the tau of lcgp_variance_reduction)
 *     L_S L_S^T = S,   v = L_S^-1 (t - ghat_k(xn))
 *   t[k, i] = psi_k . y_i / D_k with y_i the standardised output (the replicate mean on the replicated path): the entry of b_k
 *   that lcgp_nll_grad would form for that input as a training column, divided by D_k sr_i.
 * and for n0 new inputs x0:
 *     Sigma_0n = C^x(x0, xn) - D_k U_0 U_n^T   (n0 x m, no nugget),   T = Sigma_0n L_S^-T
 *     ghat'[k, :] = ghat[k, :] + T v           gvar'[k, :] = gvar[k, :] - rowsum(T o T)
 * which equals lcgp_predict(same = 0) of a model built on the augmented data at the same theta, to rounding.
 *
 *   1. lcgp_condition_prepare: the launches of lcgp_predict for xn (U_n into `state`, ghat(xn)), those of lcgp_predict_cov for
 *      S (into the matrix slot of `cond_workspace`, lcgp_workspace_bytes(dtype, m, d, p, q_local) bytes, with tau_i on the
 *      diagonal instead of a jitter), the unchanged factorisation and triangular inverse there, a dense copy of L_S^-1 into
 *      `state` with zeros above the diagonal (the product that forms T reads whole tiles), and v by one wave per row.
 *      info: q_local device ints, 0 or 1 + the first failing pivot of S (nothing is jittered; the state is then unusable).
 *      t: q_local x m doubles (device).  r: m doubles (device) or NULL (all ones).
 *   2. lcgp_condition_predict, once per chunk of new inputs: ghat / gvar by the launches of lcgp_predict(same = 0), the kernel
 *      values C^x(x0, xn), ONE launch of the MFMA tile kernel on all n0pad / 64 x mpad / 64 tiles with K = npad (operand mode
 *      OP_COND_CROSS, 64 x 64 tiles), T by the product of lcgp_predict's U, and a row reduction in lcgp_predict's order.
 * `state`: lcgp_condition_state_bytes bytes = q_local (mpad npad + mpad^2) elements + q_local mpad doubles (mpad = m rounded
 *   up to 128).  `scratch`: lcgp_condition_scratch_bytes(dtype, n, q_local, m, n0) bytes, n0 = 0 for the preparation alone
 *   (q_local mpad npad elements), otherwise the larger of that and 2 q_local n0pad (npad + mpad) elements (n0pad as in
 *   lcgp_predict); `scratch_bytes` is what the caller allocated and is checked.
 * Products in the dtype, the reductions in double, fixed order, no atomics: results are bitwise independent of the content of
 * scratch, state and cond_workspace on entry and, between calls on the same tile size (n0 below 128 in both, or not), of how a
 * caller splits the rows of x0.  They are independent of q_local as far as the factorisation and inverse of S are: those are
 * scheduled for q_local matrices of order m, and the default schedule picks 64- or 128-row tiles from q_local x the tile count
 * (lcgp_sched: syrk_small_tiles, trtri_small_tiles, trtri_level_small).  Up to mpad = 128 there is one schedule; beyond it two
 * values of q_local agree bitwise where they pick the same tile sizes, as lcgp_cv_* documents for its batch.
 * Flops per component: preparation mpad npad^2 (U_n) + mpad^2 npad (S) + mpad^3 (factor and inverse); prediction: those of
 * lcgp_predict plus 2 n0pad mpad npad (Sigma_0n) + n0pad mpad^2 (T). */
int lcgp_condition_scratch_bytes(int dtype, int n, int q_local, int m, int n0, size_t* bytes /*host out*/);
int lcgp_condition_state_bytes(int dtype, int n, int d, int q_local, int m, size_t* bytes /*host out*/);
int lcgp_condition_prepare(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                           const void* x, const void* sr, const double* theta, const void* workspace,
                           int m, const void* xn, const double* t, const double* r /*or NULL*/,
                           void* scratch, size_t scratch_bytes, void* cond_workspace, void* state, int* info);
int lcgp_condition_predict(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                           const void* x, const void* sr, const double* theta, const void* workspace,
                           const void* state, int m, const void* xn, int n0, const void* x0,
                           void* scratch, size_t scratch_bytes, double* ghat, double* gvar, int out_stride);

/* Box-averaged predictions of a conditioned view, and the covariance of every row's average with that of one reference row
 * (what lcgp_predict_marginal is to lcgp_predict, on the view or on the fitted model).  `state`, m, xn: as
 * lcgp_condition_predict takes them, or state = NULL, m = 0, xn = NULL for the fitted model; x0, mask, box: as
 * lcgp_predict_marginal takes them.  Averaging over a box is linear, so it commutes with conditioning: with Xbar the masked
 * cross rows against the training inputs and Cbar^x(x0, xn) the same masked rows against the view's inputs (no sr, no nugget
 * term; their table I1 evaluated at xn, q_local d mpad doubles),
 *     Ubar_0 = Xbar W^T        ghat, gvar: those of lcgp_predict_marginal, bitwise
 *     Sigma_0n = Cbar^x(x0, xn) - D Ubar_0 U_n^T        Tbar = Sigma_0n L_S^-T
 *     ghat' = ghat + Tbar v                             gvar' = gvar - rowsum(Tbar o Tbar)
 * Launches without a view and without a reference row: exactly those of lcgp_predict_marginal.  On a view: the table kernel
 * a second time over xn, then the masked rows against xn, OP_COND_CROSS, T and the row reduction as lcgp_condition_predict
 * enqueues them.  A row with an EMPTY mask is bitwise the row of lcgp_condition_predict on the same tile size.
 * Reference row (optional; it adds launches behind the pass and changes nothing in ghat / gvar):
 *   ref_out != NULL: the widened row [Ubar_r | Tbar_r] of pass row ref_row (0 <= ref_row < n0) is copied to ref_out,
 *     q_local x (npad + mpad) elements of the dtype (mpad = 0 without a view).
 *   ref_in != NULL: such a widened row, with the row's d values ref_x (dtype; entries under its mask are never read) and mask
 *     ref_mask (d bytes), all on the device.  gcov (q_local rows, out_stride apart as ghat) receives
 *         gcov[k, i] = prior_k(i, r) - D_k Ubar_i . Ubar_r - Tbar_i . Tbar_r
 *         prior_k(i, r) = scale_k (1 - nt_k) prod_l f_l  (ascending l):  f_l = kappa(|x0_il - ref_x_l| / ell_kl) where both rows
 *         keep l, the box average of kappa at the kept value where one of them integrates l, I2[k, l] where both do
 *     -- the covariance of the two averages of the CONTINUOUS surface (no nugget term, also between two rows with empty masks
 *     at the same input).  One wave per row (marg_refcov_kernel): lanes stride the n columns of U, then the m columns of T,
 *     sums in double in the fixed order of the row reductions; the prior is formed by lane 0 in double.
 * A caller runs a one-row pass with ref_out first and its chunked passes with ref_in afterwards; both may be given at once.
 * `scratch`: lcgp_condition_predict_marginal_scratch_bytes(dtype, n, d, q_local, m, n0) = with m = 0 that of
 * lcgp_predict_marginal, otherwise lcgp_condition_scratch_bytes of a pass + 8 q_local d (npad + 1 + mpad); checked against
 * `scratch_bytes`.  Fixed order, no atomics, one stream: bitwise independent of the scratch content on entry, of q_local in
 * lcgp_condition_predict's sense and, between calls on the same tile size, of how a caller splits the rows. */
int lcgp_condition_predict_marginal_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n0, size_t* bytes /*host out*/);
int lcgp_condition_predict_marginal(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                    const void* x, const void* sr, const double* theta, const void* workspace,
                                    const void* state /*or NULL*/, int m, const void* xn /*or NULL*/, int n0, const void* x0,
                                    const unsigned char* mask, const double* box, void* scratch, size_t scratch_bytes,
                                    double* ghat, double* gvar, int out_stride,
                                    int ref_row, void* ref_out /*or NULL*/, const void* ref_in /*or NULL*/,
                                    const void* ref_x, const unsigned char* ref_mask, double* gcov);

/* Input gradients of a conditioned view's prediction (what lcgp_predict_grad is to lcgp_predict): per local component k and
 * new input i the outputs of lcgp_condition_predict and their derivatives with respect to the standardised x0, in
 * lcgp_predict_grad's layout (dghat, dgvar: q_local x out_stride x d doubles).  `state`, m, xn: as lcgp_condition_predict takes
 * them; the workspace and the state are only read.  With T = Sigma_0n L_S^-T as there:
 *     w   = L_S^-T v                                  (m)          once per view
 *     z'  = z - D_k W^T (U_n^T w)                     (npad)       once per view        ghat' = X_0 z' + C^x(x0, xn) w
 *     R   = T L_S^-1  (= Sigma_0n S^-1)               (n0 x m)     per pass
 *     U'  = U_0 - R U_n,   V' = U' W                  (n0 x npad)  per pass
 *     dghat'[i, l] =        sum_j dc_l(x0_i, x_j) sr_j z'_j       +   sum_a dc^x_l(x0_i, xn_a) w_a
 *     dgvar'[i, l] = -2 D_k sum_j dc_l(x0_i, x_j) sr_j V'[i, j]   - 2 sum_a dc^x_l(x0_i, xn_a) R[i, a]
 * dc_l as in lcgp_predict_grad for the three kernels (0 at dx_l = 0); same = 0 throughout: the gradient of the continuous
 * surface, also at training inputs and at the view's own new inputs.
 *   1. lcgp_condition_grad_prepare, once per view: w and z' of every local component into `grad_state`
 *      (lcgp_condition_grad_state_bytes bytes = q_local (mpad + 2 npad) doubles, the second npad a work area), by three
 *      bandwidth-bound products with the transposes of L_S^-1, U_n and W, read along their rows; sums in double, the rows
 *      of a column shared among four waves in a fixed order.
 *   2. lcgp_condition_predict_grad, once per chunk of new inputs: the launches of lcgp_condition_predict (ghat' / gvar' are
 *      bitwise that function's), R over Sigma_0n by lcgp_predict_grad's product V = U W with W := L_S^-1 (64 x 64 tiles), U' in place over U_0
 *      by ONE launch of the tile kernel (operand mode OP_COND_U: K = mpad, C -= A B; 64 x 64 tiles, as OP_COND_CROSS: the 128-row
 *      instances spill in float64 and fail the counted-prefetch check in float32), V' over X as lcgp_predict_grad forms V, and lcgp_predict_grad's fused contraction over the n + m columns
 *      (pgrad_cond_kernel: the conditioning inputs are a second segment behind the training inputs, weight 1, w for z, R for
 *      V; same lane / slice / wave order, double accumulators; nothing of size n0 (n + m) d is written).
 * `scratch`: lcgp_condition_predict_grad_scratch_bytes = lcgp_condition_scratch_bytes(dtype, n, q_local, m, n0) of a pass, checked
 * against `scratch_bytes`.  Fixed order, no atomics, one stream: results are bitwise independent of the content of scratch
 * and grad_state on entry, of q_local in lcgp_condition_predict's sense, and of how a caller splits the rows of x0: R and V' are
 * formed on 64 x 64 tiles whatever n0 is (the product V = U W walks its k tiles downwards in units of the tile, so its 128-row
 * instance adds in another order; lcgp_variance_reduction_grad makes the same choice), U' likewise.
 * Flops per component beyond lcgp_condition_predict's: n0pad mpad^2 (R) + 2 n0pad mpad npad (U') + n0pad npad^2 (V'). */
int lcgp_condition_grad_state_bytes(int dtype, int n, int q_local, int m, size_t* bytes /*host out*/);
int lcgp_condition_grad_prepare(void* stream, int dtype, int n, int d, int p, int q_local, const double* theta,
                                const void* workspace, const void* state, int m, void* grad_state);
/* w (q_local x m) and z' (q_local x n) of a grad state, in double, without their padding: the weights of the view's mean surface
 * over the n + m centres are c sr_i z'_i and c w_a.  One launch; grad_state, w and z are device pointers. */
int lcgp_condition_grad_fetch(void* stream, int n, int q_local, int m, const void* grad_state, double* w, double* z);
int lcgp_condition_predict_grad_scratch_bytes(int dtype, int n, int q_local, int m, int n0, size_t* bytes /*host out*/);
int lcgp_condition_predict_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                const void* x, const void* sr, const double* theta, const void* workspace,
                                const void* state, int m, const void* xn, const void* grad_state, int n0, const void* x0,
                                void* scratch, size_t scratch_bytes, double* ghat, double* gvar, double* dghat, double* dgvar,
                                int out_stride);

/* Input Hessians and the posterior covariance of the gradient on a conditioned view (what lcgp_predict_hess and
 * lcgp_predict_gradcov are to the fitted model).  `state`, m, xn, `grad_state`: as lcgp_condition_predict_grad takes
 * them; workspace, state and grad state are only read.  Per local component k, with X_0, U_0, T, R, U', V', w, z' as there, the
 * derivative rows of lcgp_predict_hess on both column sets (their factors -1 / ell_l left out) and the row they give in the
 * augmented factor (K' = npad + mpad, the widening of lcgp_condition_vr_*):
 *     P_il   = (d_l X_i) W^T                                            (npad)
 *     Q_il   = (d_l c^x(x0_i, xn) - D_k P_il U_n^T) L_S^-T                (mpad; the launches that make T out of X_0)
 *     P'_il  = [ P_il | Q_il / sqrt(D_k) ]                              (K')
 *     d2ghat'[i, lm] =           sum_j d2c_lm(x0_i, x_j) sr_j z'_j       +   sum_a d2c^x_lm(x0_i, xn_a) w_a
 *     d2gvar'[i, lm] = -2 [ D_k sum_j d2c_lm(x0_i, x_j) sr_j V'[i, j]    +   sum_a d2c^x_lm(x0_i, xn_a) R[i, a]
 *                           + D_k P'_il . P'_im / (ell_l ell_m) ]
 *     Gamma'[i, lm]  = delta_lm c_k kappa / ell_l^2  -  D_k P'_il . P'_im / (ell_l ell_m)
 * d2c_lm, c_k, kappa as in lcgp_predict_hess / lcgp_predict_gradcov; same = 0 throughout (the Matern-3/2 psi has its kink where
 * a coordinate of x0 equals a training input's or one of the view's inputs').  Outputs in the layouts of those two functions.
 *   lcgp_condition_predict_hess: the launches of lcgp_condition_predict_grad (ghat', gvar', dghat', dgvar' are bitwise that
 *     function's; V' stays in its slab, R over Sigma_0n), then behind that pass's scratch pdx_kernel on (x0, x, sr) and on (x0, xn),
 *     P into rows K' apart (OP_PRED_U), -D P U_n^T (OP_COND_CROSS, 64 x 64 tiles), Q (OP_PRED_U on the dense L_S^-1), the tails
 *     Q / sqrt(D) behind each P row (zeros in the columns m .. mpad - 1 and in the padding rows), phess_gram_kernel over npad + m
 *     columns (the columns n .. npad - 1 of P are zero) and the two-segment contraction phess_cond_kernel (a second segment of
 *     stages over the view's inputs: weight 1, w for z, R for V; D rides on the first segment; same lane / slice / wave order,
 *     double accumulators, no atomics; nothing of size n0 (n + m) d^2 is written).
 *   lcgp_condition_predict_gradcov: dghat' by the mean-only instance of lcgp_condition_predict_grad's contraction (bitwise that
 *     function's; R, U' and V' are not formed), the rows P' as above, then gradcov_kernel and with weights gradcov_reduce_kernel
 *     over the widened rows.  gamma may be NULL when w is given; M is accumulated into (the caller carries it across passes).
 *     The per-workgroup partial sums go into the freed DX slabs: q ceil(n0 / 4) d (d + 1) / 2 doubles <= 508 q n0 d bytes, less
 *     than the q rows_pad npad elements there, as in lcgp_predict_gradcov.
 * `scratch`: lcgp_condition_predict_hess_scratch_bytes = that of lcgp_condition_predict_grad + q rows_pad (2 K' + mpad) elements
 * (P', DX, the derivative rows against xn and Q); lcgp_condition_predict_gradcov_scratch_bytes = q rows_pad (2 K' + mpad)
 * elements (rows_pad = n0 d padded as in lcgp_predict_hess); both
 * checked against `scratch_bytes`.  n0 d <= LCGP_HESS_MAX_ROWS.  Fixed order, one stream: results are bitwise independent of the
 * content of scratch on entry and of q_local.
 * Flops per component beyond lcgp_predict_hess's: rows_pad mpad (2 npad + mpad) for Q. */
int lcgp_condition_predict_hess_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n0, size_t* bytes /*host out*/);
int lcgp_condition_predict_hess(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                const void* x, const void* sr, const double* theta, const void* workspace,
                                const void* state, int m, const void* xn, const void* grad_state, int n0, const void* x0,
                                void* scratch, size_t scratch_bytes, double* ghat, double* gvar, double* dghat, double* dgvar,
                                double* d2ghat, double* d2gvar, int out_stride);
int lcgp_condition_predict_gradcov_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n0, size_t* bytes /*host out*/);
int lcgp_condition_predict_gradcov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                   const void* x, const void* sr, const double* theta, const void* workspace,
                                   const void* state, int m, const void* xn, const void* grad_state, int n0, const void* x0,
                                   void* scratch, size_t scratch_bytes, double* dghat, double* gamma /*or NULL*/,
                                   const double* w /*or NULL*/, double* M /*or NULL*/, int out_stride);

/* Closed-form cross-validation at fixed parameters (no counterpart in the reference).  Input: the workspace of the last
 * lcgp_nll_grad, whose V slot holds a = A_k^-1 (A_k = I + D_k (C_k o s s^T), s = sr, ones when sr is NULL) and whose vectors
 * hold b_k and z_k = A_k^-1 b_k.  With K_k = C_k + (D_k S^2)^-1 (S = diag(s)), K_k^-1 = D_k S a S, so for a set B of m
 * training inputs and M = a[B, B] (m x m) the model conditioned on the OTHER inputs -- same theta, D_k, psi_k, basis and
 * standardisation, no nugget in the cross covariance (same = 0) -- predicts at x_B
 *     ghat_B  = S_B^-1 (b_B - M^-1 z_B) / D_k
 *     Sigma_B = S_B^-1 (M^-1 - I) S_B^-1 / D_k        (the prior variance scale_k, nugget included, on its diagonal)
 * and leave-one-out (B = {i}) is
 *     ghat_i = (b_i - z_i / a_ii) / (D_k s_i),   gvar_i = (1 / a_ii - 1) / (D_k s_i^2).
 * These equal lcgp_predict of the conditioned model at x_B to rounding: no refit, no factorisation of size n.
 *
 * lcgp_loo: ghat / gvar for every training input, q_local rows of n doubles `out_stride` apart (0 = n).  Bitwise independent
 * of q_local; accumulates in double.
 *
 * k-fold: the folds are given twice -- `folds_host` (host) and `folds` (device) hold the same F + 1 + n ints
 *     [ fold_ptr_0 .. fold_ptr_F | fold_idx_0 .. fold_idx_{n-1} ],   fold f = fold_idx[fold_ptr_f .. fold_ptr_{f+1}),
 * a partition of 0 .. n-1 into F non-empty folds, each sorted ascending.  The host copy is checked before anything is
 * enqueued (an empty fold, an index out of range or repeated, fold_ptr not running from 0 to n, F * q_local > 65535 and
 * NULL pointers are refused); the kernels read the device copy.  mmax = the largest fold.
 *   1. lcgp_cv_gather writes M = a_k[B_f, B_f] into the matrix slot f * q_local + k of a SECOND workspace, `cv_workspace`,
 *      of lcgp_cv_workspace_bytes bytes (= lcgp_workspace_bytes(dtype, mmax, d, p, q_local * F)): lower 64x64 tiles,
 *      identity beyond m_f -- what lcgp_potrf_logdet(dtype, mmax, d, p, q_local * F, cv_workspace, ...) factors in place.
 *   2. the caller factors and inverts with the existing entries: lcgp_potrf_logdet (a plan with with_inverse = 0; its info
 *      word of slot f * q_local + k reports a fold matrix that is not numerically positive definite), then lcgp_potri.
 *      M^-1 is then in the V slot (lcgp_fetch_matrix(..., which = 2, f * q_local + k) for Sigma_B).
 *   3. lcgp_cv_apply forms t = M^-1 z_B and scatters ghat / gvar of every fold to the positions fold_idx of q_local rows of
 *      n doubles, `out_stride` apart.  Fixed-order sums, no atomics: bitwise reproducible run to run (not across q_local:
 *      the schedule of step 2 depends on the batch q_local * F).
 * The content of `cv_workspace` on entry is irrelevant.  Memory: 3 q_local F mpad^2 elements (mpad = mmax rounded up to
 * 128); flops per slot: mpad^3 / 3 (factor) + 2 mpad^3 / 3 (inverse) + 2 mmax^2 (apply). */
int lcgp_loo(void* stream, int dtype, int n, int d, int p, int q_local, const void* sr, const double* theta,
             const void* workspace, double* ghat, double* gvar, int out_stride);
int lcgp_cv_workspace_bytes(int dtype, int n, int d, int p, int q_local, int F, const int* folds_host, size_t* bytes /*host out*/);
int lcgp_cv_gather(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace, int F,
                   const int* folds_host, const int* folds, void* cv_workspace);
int lcgp_cv_apply(void* stream, int dtype, int n, int d, int p, int q_local, const void* sr, const double* theta,
                  const void* workspace, int F, const int* folds_host, const int* folds, const void* cv_workspace,
                  double* ghat, double* gvar, int out_stride);

/* Integrated variance reduction at fixed parameters (the active-learning-Cohn criterion, ALC / IMSPE reduction; no counterpart
 * in the reference).  Input: the workspace of the last lcgp_nll_grad, as for lcgp_predict.  With X_k = c0k o sr^T and
 * U_k = X_k L_k^-T exactly as in lcgp_predict, for local component k, reference point t and candidate c (both standardised):
 *     out[k, c]       = sum_t w_t Sigma_k(t, c)^2 / (max(Sigma_k^h(c, c), 0) + 1 / (D_k r))
 *     Sigma_k(t, c)   = C_k(t, c) - D_k U_k(t) . U_k(c)      C_k without nugget: reference points are new inputs (same = 0)
 *     Sigma_k^h(c, c) = scale_k - D_k |U_k(c)|^2             = lcgp_predict's gvar at c with the candidate's own cross row
 * i.e. the drop of sum_t w_t gvar_k(t) if the training set were augmented by r replicates at c (same theta, A refactorised).
 * A candidate's cross row has no nugget term unless match[c] = i >= 0: c IS training input i (the replicated path: it adds r
 * replicates to input i) and the term scale_k nug sr_i goes to column i (lcgp_predict's `same` convention, per row).
 * The caller normalises w; reference rows beyond n_ref count with weight 0.
 *
 *   1. lcgp_variance_reduction_prepare forms U_k and gvar_k of the n_ref reference points into `scratch` (the reference part).
 *   2. lcgp_variance_reduction, once per chunk of candidates, reads that part: it forms U_k and gvar_k of the candidates (or,
 *      with cand_row0 >= 0, takes rows cand_row0 .. cand_row0 + n_cand - 1 of the reference set's: the candidates ARE those
 *      reference points; x_cand, match_host and match are then NULL), then runs ONE launch of the MFMA tile kernel over the
 *      (reference tile, candidate tile) pairs whose epilogue recomputes C_k from x_ref / x_cand, forms Sigma_k and reduces
 *      w_t Sigma_k^2 / den_c over the tile's rows (the n_ref x n_cand matrix never reaches memory), and a reduction over the
 *      reference tiles in ascending order (no atomics).  out: q_local rows of n_cand doubles, `out_stride` apart (0 = n_cand).
 *      Bitwise independent of q_local and of how candidates are split over calls.  Products in the dtype, sums in double.
 *   match_host / match: the same n_cand ints (host, checked before anything is enqueued; device, read by the kernels), each -1
 *      or a training index in [0, n); both NULL = no matches.  w_ref: n_ref doubles (device).  r >= 1.
 * scratch: lcgp_variance_reduction_scratch_bytes(dtype, n, q_local, n_ref, n_cand) bytes -- q_local (n_ref + n_cand) npad
 *   elements for the two U plus X work areas of at most 2048 rows each and q_local ceil(n_ref / 64) n_cand doubles of partial
 *   sums; a scratch sized for n_cand serves calls with fewer candidates.  Its content on entry to step 1 is irrelevant; step 2
 *   reads the reference part step 1 wrote (same n, q_local, theta, workspace, n_ref, x_ref) and writes everything else it reads.
 * Flops per component: n_refpad npad^2 (U of the reference set, once; 2 per multiply-add over the lower triangle of L^-1) +
 *   n_candpad npad^2 (U of the candidates, unless cand_row0 >= 0) + 2 n_ref64 n_cand64 npad (the fused product); n_refpad /
 *   n_candpad: rounded up to 128 (to 64 below 128), n_ref64 / n_cand64: rounded up to 64. */
int lcgp_variance_reduction_scratch_bytes(int dtype, int n, int q_local, int n_ref, int n_cand, size_t* bytes /*host out*/);
int lcgp_variance_reduction_prepare(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                    const void* x, const void* sr, const double* theta, const void* workspace,
                                    int n_ref, const void* x_ref, void* scratch);
int lcgp_variance_reduction(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                            const void* x, const void* sr, const double* theta, const void* workspace,
                            int n_ref, const void* x_ref, const double* w_ref,
                            int n_cand, const void* x_cand, const int* match_host /*host or NULL*/, const int* match,
                            int cand_row0, int r, void* scratch, double* out, int out_stride);

/* Gradient of the integrated variance reduction with respect to the candidate's location (standardised scale; no counterpart in
 * the reference).  Every candidate is a NEW input (no match): with R = N / den the result of lcgp_variance_reduction,
 *     dout[k, c, l] = (d_l N - R d_l h) / den
 *     d_l h(c) = -2 D_k sum_j dc_l(c, j) sr_j V_k[c, j],   V_k = U_cand W_k      (lcgp_predict_grad's dgvar; taken as 0 where h <= 0)
 *     d_l N(c) = 2 [ sum_t dC_l(c, t) S[c, t] - D_k sum_j dc_l(c, j) sr_j Q[c, j] ],   S[c, t] = w_t Sigma_k(t, c),  Q = (S U_ref) W_k
 * with dc_l the first kernel derivative of lcgp_predict_grad (no nugget term).  x_ref and w_ref are constants, also where the
 * candidates are rows of the reference set (cand_row0 >= 0).
 * Runs behind lcgp_variance_reduction_prepare (same scratch, sized by lcgp_variance_reduction_grad_scratch_bytes), once per
 * chunk of candidates: the launches of lcgp_variance_reduction (out: bitwise its result), then P = U_cand U_ref^T and G = S U_ref
 * on the MFMA tile kernel, S from P in place (C recomputed in double), Q and V (the product of lcgp_predict_grad), the fused
 * contraction of lcgp_predict_grad over the reference points (S) and over the training inputs (Q beside V), and one combining
 * launch.  Products in the dtype; Sigma, sums and contractions in double, in a fixed order, no atomics: bitwise independent of
 * q_local, of the scratch content and of how the candidates are split over calls.
 * out: q_local rows of n_cand doubles, out_stride apart (0 = n_cand); dout: [q_local][out_stride][d] doubles.
 * scratch: that of lcgp_variance_reduction plus q_local n_candpad (n_refpad + 2 npad) elements (S, G / V, Q) and 3 q_local
 *   n_cand d doubles; n_candpad / n_refpad rounded up to 128 (n_candpad to 64 below 128).  n_cand <= 65407 per call.
 * Flops per component beyond lcgp_variance_reduction: 4 n_candpad n_refpad npad (P, G) + 2 n_candpad npad^2 (Q, V). */
int lcgp_variance_reduction_grad_scratch_bytes(int dtype, int n, int d, int q_local, int n_ref, int n_cand,
                                               size_t* bytes /*host out*/);
int lcgp_variance_reduction_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                 const void* x, const void* sr, const double* theta, const void* workspace,
                                 int n_ref, const void* x_ref, const double* w_ref,
                                 int n_cand, const void* x_cand, int cand_row0, int r, void* scratch,
                                 double* out, int out_stride, double* dout);

/* Greedy batch design by sequential ALC at fixed parameters (no counterpart in the reference): pick the candidate with the
 * largest score, condition the posterior covariance on r runs there (ALC does not depend on the runs' outputs), score again.
 * Per local component k, with Sigma, Sigma^h, den as in lcgp_variance_reduction and R_k = N_k / den_k its result:
 *     score(c) = sum_k omega_k R_k(c)        over the local components in ascending order (rounded products and sums),
 *                                            -inf at candidates already picked
 *   pick j:  pcol = Sigma_k(cand, j),  scol = Sigma_k(ref, j)  of the CURRENT posterior:
 *              C^x(., j) - D_k U_k(.) . U_k(j) - sum_{s<t} hist[s, .] V[s, j]          (C^x: kernel without nugget)
 *            v = pcol / sqrt(den_k(j)),  u = scol / sqrt(den_k(j)),  V[t, :] = v,  Uh[t, :] = u
 *            g = C^x(cand, ref) (w o u) - D_k U_cand (U_ref^T (w o u)) - sum_{s<t} V[s, :] (Uh[s, :] . (w o u))
 *            N <- max(N - 2 v o g + v o v (u . (w o u)), 0),   h <- h - v o v,   R <- N / (max(h, 0) + 1 / (D_k r))
 * a pivoted Cholesky of the posterior covariance over the candidates carried lazily: nothing of size n_ref x n_cand or
 * n_cand x n_cand is stored.  Two different points never share a nugget: the caller refuses duplicate candidates.
 *
 *   1. lcgp_select_begin forms U_k / gvar_k of the reference set and of ALL candidates (resident in `scratch`; candidates pass
 *      through the one X work area `pass_rows` <= 2048 rows at a time), then R_k with the launches of lcgp_variance_reduction:
 *      bitwise what that entry writes for the same sets.  match_host / match, w_ref, r as there.  h_k = gvar_k of the candidates.
 *   2. lcgp_select_score writes the score row of step `step` to out (n_cand doubles, device; NULL = not wanted) and the argmax
 *      (lowest index wins ties) into the device word picks[step] of the scratch (lcgp_select_picks returns the address of picks).
 *      omega: q_local doubles (device).
 *   3. lcgp_select_condition performs the step above for the pick it reads from DEVICE memory (`pick`: picks + step, or any
 *      device int the caller wrote), for all local components, and marks the candidate picked.  Steps 2 and 3 for step = 0 ..
 *      size - 1 can be enqueued back to back without a host synchronisation.  Five launches: (i) one wave per row of
 *      [U_cand; U_ref] . U_cand[j] (K = n) with the kernel value, the history correction and the scaling in its epilogue;
 *      (ii) y = U_ref^T (w o u) over fixed chunks of 32 reference rows, the chunks' partials summed in ascending order (no
 *      atomics), and the history dot products; (iii) one wave per candidate: U_cand y, the on-the-fly C^x(cand, ref) (w o u) and
 *      the update of N / h.  16-byte loads, double accumulation in both dtypes (float32: U is float32, all else double).
 *   lcgp_select_state copies R (which = 0) or h (which = 1), q_local rows of n_cand doubles, to `out` (device).
 * Results are bitwise independent of the scratch content on entry to step 1, of q_local and of pass_rows.
 * scratch: lcgp_select_scratch_bytes bytes -- q_local (n_ref + n_cand) npad elements for the two U, one X work area of at most
 *   2048 rows, the partial sums of lcgp_variance_reduction for all candidates, and in double: R, h, V (size x n_cand), Uh (size x
 *   n_ref), ceil(n_ref / 32) npad partials of y, the inputs divided by ell (q_local (n_ref + n_cand) d), the score state.
 * Traffic per step and component: U_ref and U_cand twice each. */
int lcgp_select_scratch_bytes(int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, size_t* bytes /*host out*/);
int lcgp_select_begin(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                      const void* x, const void* sr, const double* theta, const void* workspace,
                      int n_ref, const void* x_ref, const double* w_ref,
                      int n_cand, const void* x_cand, const int* match_host /*host or NULL*/, const int* match,
                      int r, int size, int pass_rows, void* scratch);
int lcgp_select_score(void* stream, int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, int step,
                      const double* omega, void* scratch, double* out /*device or NULL*/);
int lcgp_select_picks(int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, void* scratch, int** picks /*host out*/);
int lcgp_select_condition(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* theta,
                          int n_ref, int n_cand, int size, int r, int step, const int* pick /*device*/, void* scratch);
int lcgp_select_state(void* stream, int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, int which,
                      const void* scratch, double* out);

/* Variance reduction and greedy selection on a CONDITIONED VIEW (no counterpart in the reference): lcgp_variance_reduction and
 * lcgp_select_* of the model lcgp_condition_prepare conditioned on m new inputs xn, without refactorising -- what closes the
 * loop pick a batch / run the simulator / lcgp_condition_prepare / pick the next batch.  `state`, m, xn: as
 * lcgp_condition_predict takes them; the workspace and the state are only read.  For any input a, with U_a as in lcgp_predict
 * and the notation of lcgp_condition_*:
 *     Sigma_an = C^x(a, xn) - D_k U_a U_n^T,   T_a = Sigma_an L_S^-T         (1 x mpad, zero beyond m)
 *     Sigma'_k(t, c)   = C_k(t, c) - D_k U_t . U_c - T_t . T_c                 (the view's posterior covariance)
 *     Sigma'^h_k(c, c) = gvar_k(c) - |T_c|^2                                   (lcgp_condition_predict's gvar)
 * With the WIDENED ROW U^_a = [U_a | T_a / sqrt(D_k)] of length K' = npad + mpad (mpad = m rounded up to 128) these are
 * C_k - D_k U^_t . U^_c and scale_k - D_k |U^_c|^2: the forms lcgp_variance_reduction and lcgp_select_* consume, so
 *     out[k, c] = sum_t w_t Sigma'_k(t, c)^2 / (max(Sigma'^h_k(c, c), 0) + 1 / (D_k r))
 * equals lcgp_variance_reduction of a model built on the augmented data at the same theta, to rounding, and the selection is
 * lcgp_select_* on widened rows.  A candidate must not equal a conditioning input (the caller refuses it); match, w_ref, r,
 * cand_row0, pass_rows, omega, step, pick, which and the outputs are those of the entry each one mirrors.
 *
 * The row former, for a block of at most 2048 inputs: the launches of lcgp_variance_reduction's (cross rows with the match
 * term, U into rows K' apart, gvar), then those of lcgp_condition_predict on the block (the kernel values C^x(., xn), Sigma_an by
 * OP_COND_CROSS, T by the product of lcgp_predict's U on the dense L_S^-1), and one launch that writes T / sqrt(D_k) behind the
 * row's U -- zeros in columns m .. mpad - 1 and in the rows of the padding, whatever the scratch held -- and takes rowsum(T o T)
 * off gvar in lcgp_condition_predict's order: for a row without a match gvar is bitwise lcgp_condition_predict's.  The fused
 * product (OP_VR) then runs with K = K', the selection's row kernels with row length and dot length K'.
 *
 * scratch (`scratch_bytes` is what the caller allocated and is checked by every entry), with esz the element size, npad / mpad
 * n / m rounded up to 128, pad(v) = v rounded up to 128 (to 64 below 128) and every part rounded up to 256 bytes:
 *   lcgp_condition_vr_scratch_bytes:  reference part  q (pad128(n_ref) + 64) K' esz + 2 q n_ref 8 + q X_r npad esz + 2 q X_r mpad esz,
 *        X_r = min(2048, pad(n_ref));  candidate part  q pad(n_cand) K' esz + 2 q n_cand 8 + q X_c npad esz + 2 q X_c mpad esz
 *        + q ceil(n_ref / 64) pad64(n_cand) 8,  X_c = min(2048, pad(n_cand))       (pad128 / pad64: rounded up to 128 / 64)
 *   lcgp_condition_select_scratch_bytes:  q (pad128(n_ref) + 64) K' esz + q (pad(n_cand) + 128) K' esz + q X npad esz + 2 q X mpad esz
 *        (X = min(2048, max(pad(n_ref), pad(n_cand)))) + doubles: q (2 n_ref + 2 n_cand) + q ceil(n_ref / 64) pad64(n_cand) + q n_cand
 *        + q size (n_cand + n_ref) + q ceil(n_ref / 32) K' + q K' + q size + q (n_ref + n_cand) d + n_ref, and n_cand + size ints.
 *   A scratch sized for n_cand serves lcgp_condition_vr calls with fewer candidates.
 * Numerics follow lcgp_variance_reduction: products in the dtype, Sigma, sums and reductions in double, fixed order, no
 * atomics.  Results are bitwise independent of the content of scratch on entry, of q_local, of how candidates are split over
 * calls and of pass_rows.  The entries of the fitted model run the same code with K = npad and are bitwise what they were.
 * Flops per component beyond the base entries', per row of either set: 2 mpad npad (Sigma_an) + mpad^2 (T); the fused product
 * is 2 n_ref64 n_cand64 K'. */
int lcgp_condition_vr_scratch_bytes(int dtype, int n, int q_local, int m, int n_ref, int n_cand, size_t* bytes /*host out*/);
int lcgp_condition_vr_prepare(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                              const void* x, const void* sr, const double* theta, const void* workspace,
                              const void* state, int m, const void* xn,
                              int n_ref, const void* x_ref, void* scratch, size_t scratch_bytes);
int lcgp_condition_vr(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                      const void* x, const void* sr, const double* theta, const void* workspace,
                      const void* state, int m, const void* xn,
                      int n_ref, const void* x_ref, const double* w_ref,
                      int n_cand, const void* x_cand, const int* match_host /*host or NULL*/, const int* match,
                      int cand_row0, int r, void* scratch, size_t scratch_bytes, double* out, int out_stride);
int lcgp_condition_select_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size,
                                        size_t* bytes /*host out*/);
int lcgp_condition_select_begin(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                const void* x, const void* sr, const double* theta, const void* workspace,
                                const void* state, int m, const void* xn,
                                int n_ref, const void* x_ref, const double* w_ref,
                                int n_cand, const void* x_cand, const int* match_host /*host or NULL*/, const int* match,
                                int r, int size, int pass_rows, void* scratch, size_t scratch_bytes);
int lcgp_condition_select_score(void* stream, int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size,
                                int step, const double* omega, void* scratch, size_t scratch_bytes, double* out /*device or NULL*/);
int lcgp_condition_select_picks(int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size, void* scratch,
                                size_t scratch_bytes, int** picks /*host out*/);
int lcgp_condition_select_condition(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* theta,
                                    int m, int n_ref, int n_cand, int size, int r, int step, const int* pick /*device*/,
                                    void* scratch, size_t scratch_bytes);
int lcgp_condition_select_state(void* stream, int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size,
                                int which, const void* scratch, size_t scratch_bytes, double* out);

/* Gradient of the variance reduction on a CONDITIONED VIEW with respect to the candidate's location (standardised scale; no
 * counterpart in the reference): lcgp_variance_reduction_grad of the model lcgp_condition_prepare conditioned on m new inputs
 * xn, without refactorising.  `state`, m, xn as lcgp_condition_vr takes them; every other argument as
 * lcgp_variance_reduction_grad's; the workspace and the state are only read.  Every candidate is a NEW input (no match).  With
 * the widened rows U^_a = [U_a | T_a / sqrt(D_k)] of length K' = npad + mpad, Sigma', h' = Sigma'^h and den' as in lcgp_condition_vr,
 * R' = N' / den' its result and S'[c, t] = w_t Sigma'_k(t, c):
 *     t1[c, l]  = sum_t dC_l(c, t) S'[c, t]
 *     G^        = S' U^_ref = [G_U | G_T / sqrt(D_k)]                           (n_cand x K')
 *     Q_n       = G_T L_S^-1,      Q'   = (G_U - Q_n U_n) W_k
 *     R_c       = T_c L_S^-1,      V'_c = (U_c - R_c U_n) W_k                   (lcgp_condition_predict_grad's R and V')
 *     a1[c, l]  = D_k sum_j dc_l(c, j) sr_j Q'[c, j] + sum_a dc^x_l(c, xn_a) Q_n[c, a]
 *     d_l h'(c) = -2 D_k sum_j dc_l(c, j) sr_j V'_c[c, j] - 2 sum_a dc^x_l(c, xn_a) R_c[c, a]        (taken as 0 where h' <= 0)
 *     dout[k, c, l] = (2 (t1 - a1) - R' d_l h') / den'
 * which equals lcgp_variance_reduction_grad of a model built on the augmented data at the same theta, to rounding.
 * Runs behind lcgp_condition_vr_prepare (same scratch, sized by lcgp_condition_vr_grad_scratch_bytes), once per chunk of
 * candidates: the launches of lcgp_condition_vr without a match (out: bitwise its result), P' = U^_cand U^_ref^T (K = K') and S'
 * from it in place, t1 by the fused contraction over the reference points, G^ over K' columns, Q_n and R_c by the product of
 * lcgp_condition_predict_grad's R on the dense L_S^-1 (rows K' apart in, mpad apart out) and one scaling launch each (the tails
 * carry 1 / sqrt(D_k)), G_U - Q_n U_n in place and U_c - R_c U_n in a buffer of its own (the candidates' rows may be rows of
 * U^_ref), Q' and V'_c by the product of lcgp_predict_grad, ONE fused contraction over the n + m columns with a matrix in the
 * place of z in both segments (Q' beside V'_c over the training inputs, Q_n beside R_c over the conditioning inputs), and the
 * combining launch.  64-row tiles for every product whose rows are candidates.  Products in the dtype; Sigma', sums and
 * contractions in double, in a fixed order, no atomics, one stream: bitwise independent of q_local, of the scratch content and
 * of how the candidates are split over calls.  lcgp_variance_reduction_grad runs the same code with K = npad and is bitwise what
 * it was.
 * scratch (`scratch_bytes` is checked before anything is enqueued): lcgp_condition_vr_scratch_bytes(dtype, n, q_local, m, n_ref,
 *   n_cand) plus, with C = pad(n_cand), esz, npad, mpad, pad() as there and every part rounded up to 256 bytes:
 *     q C pad128(n_ref) esz (S')  +  q C K' esz (G^ / V'_c)  +  q C npad esz (Q')  +  3 q n_cand d 8 (t1, a1, d h')
 *     +  q C npad esz (U_c - R_c U_n)  +  2 q C mpad esz (Q_n, R_c)
 *   With mpad = 0 the two sums are lcgp_variance_reduction_grad_scratch_bytes.  n_cand <= 65407 per call.
 * Flops per component beyond lcgp_condition_vr: 4 C pad128(n_ref) K' (P', G^) + 2 C npad^2 (Q', V'_c) + 2 C mpad^2 (Q_n, R_c)
 *   + 4 C mpad npad (the two products with U_n). */
int lcgp_condition_vr_grad_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand,
                                         size_t* bytes /*host out*/);
int lcgp_condition_vr_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                           const void* x, const void* sr, const double* theta, const void* workspace,
                           const void* state, int m, const void* xn,
                           int n_ref, const void* x_ref, const double* w_ref,
                           int n_cand, const void* x_cand, int cand_row0, int r, void* scratch, size_t scratch_bytes,
                           double* out, int out_stride, double* dout);

/* Joint posterior covariance of a conditioned view over new inputs (no counterpart in the reference): lcgp_predict_cov of the
 * model lcgp_condition_prepare conditioned on m new inputs xn, without refactorising.  `state`, m, xn: as lcgp_condition_predict
 * takes them; the workspace and the state are only read.  With the widened row U^_a = [U_a | T_a / sqrt(D_k)] of length
 * K' = npad + mpad (lcgp_condition_vr above), for local component k and n0 new inputs x0 (standardised):
 *     Sigma'_k = C00_k - D_k U^ U^^T  =  C00_k - D_k U_0 U_0^T - T T^T          (n0 x n0),   T = Sigma_0n L_S^-T
 *     diag(Sigma'_k) = gvar'[k, :] of lcgp_condition_predict, to rounding
 *     C00_k = the covariance kernel of x0 with itself, nugget on the diagonal (lcgp_predict_cov's)
 * which equals lcgp_predict_cov(same = 0) of a model built on the augmented data at the same theta, to rounding.  Rows of x0
 * that equal training inputs or conditioning inputs get the continuous surface (no match term, same = 0: lcgp_condition_predict's
 * rule).  The result goes where lcgp_predict_cov puts it: the matrix slot of `cov_workspace`
 * (lcgp_workspace_bytes(dtype, n0, d, p, q_local) bytes) holds Sigma'_k + tau_k I, tau_k = jitter * scale_k, lower tiles valid,
 * identity on the padding; lcgp_potrf_logdet factors it there and lcgp_sample_latent draws from the factor, both unchanged (the
 * mean of the draws: ghat' of lcgp_condition_predict).
 * Launches, all local components each, one stream:
 *   1. the row former of lcgp_condition_vr (no match) on blocks of at most 2048 rows of x0, into a slab of n0pad x K' elements
 *      per component (n0pad = n0 rounded up to 128).  A last block of fewer than 128 rows is padded to 64 by the row former: the
 *      up to 64 rows of the slab behind it are zeroed by one small launch (the product reads whole tiles);
 *   2. C00_k into the matrix slot (the launch of lcgp_predict_cov);
 *   3. ONE launch of the tile kernel over the lower tiles, C00_k -= D_k U^ U^^T (operand mode OP_PRED_COV, 64 x 64 tiles, rows
 *      K' apart, K = K': the instance lcgp_predict_cov runs with K = npad);
 *   4. the diagonal: + tau_k on rows below n0, 1 on the padding (the launch of lcgp_predict_cov).
 * scratch: lcgp_condition_predict_cov_scratch_bytes(dtype, n, q_local, m, n0) bytes =
 *     q n0pad K' esz  +  q X npad esz  +  2 q X mpad esz  +  2 roundup256(q n0 8),      X = min(2048, pad(n0)),
 * esz the element size, pad(v) = v rounded up to 128 (to 64 below 128), every part rounded up to 256 bytes; `scratch_bytes` is
 * what the caller allocated and is checked before anything is enqueued.
 * Products in the dtype, the row sums in double, fixed order, no atomics: the result is bitwise independent of the content of
 * scratch and cov_workspace on entry, and of q_local in lcgp_condition_predict's sense (the state is what depends on it).
 * Flops per component: those of lcgp_predict_cov (n0pad^2 npad + n0pad npad^2 / 2) plus 2 n0pad mpad npad + n0pad mpad^2 for
 * the rows (Sigma_0n and T) and n0pad^2 mpad for the wider product. */
int lcgp_condition_predict_cov_scratch_bytes(int dtype, int n, int q_local, int m, int n0, size_t* bytes /*host out*/);
int lcgp_condition_predict_cov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                               const void* x, const void* sr, const double* theta, const void* workspace,
                               const void* state, int m, const void* xn, int n0, const void* x0,
                               void* scratch, size_t scratch_bytes, void* cov_workspace, double jitter);

/* Calibration rows (no counterpart in the reference): the log density of ONE observation vector of the outputs given the
 * latent prediction of each of n0 inputs, and its derivatives.  With Phi_s the (scaled) output map restricted to the observed
 * outputs, t the centred observation and Lambda the input-independent part of the covariance (noise + observation covariance),
 * the caller folds everything output-sized ONCE into
 *     M = Phi_s^T Lambda^-1 Phi_s (q x q, symmetric),  b = Phi_s^T Lambda^-1 t,  c0 = t^T Lambda^-1 t,
 *     lognorm = logdet Lambda + |O| log 2 pi
 * and per row i, with g = ghat[:, i] and h = sqrt(max(gvar[:, i], 0)):
 *     w = b - M g,   K = I + diag(h) M diag(h) = L L^T   (eigenvalues >= 1: never fails for finite input),   u = L^-1 (h o w)
 *     ll[i] = -1/2 (c0 - 2 b.g + g^T M g - u.u + 2 sum_k log L_kk + lognorm)
 *           = log N(y_obs; Phi_s g, Phi_s diag(gvar) Phi_s^T + Lambda)
 *     s = w - M (h o L^-T u) = d ll / d ghat,   R = L^-1 diag(h) M,   v_k = 1/2 s_k^2 - 1/2 (M_kk - sum_j R_jk^2) = d ll / d gvar_k
 *     dll[i, l] = inv_range[l] sum_k (s_k dghat[k, i, l] + v_k dgvar[k, i, l])
 * (no division by gvar anywhere: rows with gvar = 0 are ordinary).  ghat, gvar, dghat, dgvar are the double arrays lcgp_predict /
 * lcgp_predict_grad write, for models of either precision; q is the TOTAL number of components (the q x q system couples them).
 * One launch: q <= 8 one thread per row with every component loop unrolled, 8 < q <= 64 one wavefront per row with the factor
 * in 16 q^2 bytes of LDS.  float64, no atomics, fixed summation order: a row's results are bitwise reproducible, independent of
 * the content of the outputs on entry and of how a caller splits the rows over calls.  Arguments are checked before any launch. */
#define LCGP_CALIB_MAX_Q 64
int lcgp_calib_rows(void* stream, int q, int d, int n0,
                    const double* ghat, const double* gvar,      /* q rows of n0, in_stride apart (0 = n0) */
                    const double* dghat, const double* dgvar,    /* q x n0 x d, row k at k * in_stride * d; both NULL: no gradient */
                    int in_stride,
                    const double* M /* q x q, device */, const double* b /* q, device */, double c0, double lognorm,
                    const double* inv_range /* d, device; NULL = ones */,
                    double* ll /* n0 */, double* dll /* n0 x d or NULL */, double* sens /* 2 x q x n0 (s then v) or NULL */);

/* Calibration rows to second order: lcgp_calib_rows plus the Hessian of ll[i] in the row's input.  With
 *     B = M - R^T R     (= Phi_s^T Sigma_i^-1 Phi_s, q x q symmetric; v_k = 1/2 s_k^2 - 1/2 B_kk)
 * the second derivatives of ll in the latents are
 *     d2 ll / d ghat_k d ghat_j = -B_kj,   d2 ll / d ghat_k d gvar_j = -B_kj s_j,   d2 ll / d gvar_k d gvar_j = 1/2 B_kj^2 - s_k s_j B_kj
 * and with P = dghat[:, i, :], V = dgvar[:, i, :] (q x d) and the packed Hessians of lcgp_predict_hess (entry (l, m <= l) at
 * l (l + 1) / 2 + m, tri = d (d + 1) / 2 per row)
 *     d2ll[i, lm] = inv_range_l inv_range_m ( sum_k s_k d2ghat[k, i, lm] + v_k d2gvar[k, i, lm]
 *                     - (P^T B P)_lm - (P^T B diag(s) V)_lm - (P^T B diag(s) V)_ml + (V^T (1/2 B o B - (s s^T) o B) V)_lm )
 * packed the same way.  No division by gvar: rows with gvar = 0 or slightly below are ordinary rows.
 * Two launches on one stream: lcgp_calib_rows' own launch writes ll, dll and sens, so these are BITWISE lcgp_calib_rows' for
 * every q; then one wavefront per row (any q in [1, 64], 16 q^2 bytes of LDS) refactorises K, forms R, s, v and B (in L's
 * place) and contracts column by column of the triangle: O(q^3 + q^2 d + q d^2) per row.  The second launch reads none of the
 * first one's outputs and runs when d2ll or Bout is given.  float64, no atomics, fixed summation order: a row's results are
 * bitwise independent of the content of the outputs on entry, of how a caller splits the rows over calls and of which optional
 * outputs are requested.  Limits and checks are lcgp_calib_rows'; arguments are checked before any launch. */
int lcgp_calib_hess_rows(void* stream, int q, int d, int n0,
                         const double* ghat, const double* gvar,      /* q rows of n0, in_stride apart (0 = n0) */
                         const double* dghat, const double* dgvar,    /* q x n0 x d, row k at k * in_stride * d */
                         const double* d2ghat, const double* d2gvar,  /* q x n0 x tri, row k at k * in_stride * tri; needed for d2ll */
                         int in_stride,
                         const double* M /* q x q, device */, const double* b /* q, device */, double c0, double lognorm,
                         const double* inv_range /* d, device; NULL = ones */,
                         double* ll /* n0 */, double* dll /* n0 x d or NULL */, double* d2ll /* n0 x tri or NULL */,
                         double* sens /* 2 x q x n0 (s then v) or NULL */, double* Bout /* n0 x q x q or NULL */);

/* Pair sums behind the closed-form Sobol indices of the posterior mean surface.  Component k's surface is
 *     ghat_k(t) = sum_i w[k, i] prod_l kappa(|t_l - x[i, l]| / ell[k, l])
 * (w = scale (1 - nt) sr o z, what the box-averaged prediction multiplies its rows by).  With, per input dimension l,
 *     a_l[i]     = (1 / w_l) int_box kappa(|t - x_il| / ell_kl) dt                                    (component k;  a'_l: k')
 *     J_l[i, i'] = (1 / w_l) int_box kappa(|t - x_il| / ell_kl) kappa(|t - x_i'l| / ell_k'l) dt
 *     M_u[i, i'] = prod_{l in u} J_l[i, i'] prod_{l not in u} a_l[i] a'_l[i']                         (M_0: u empty)
 * row r of `out` holds, for the pair (k, k') = (pairs[2 r], pairs[2 r + 1]),
 *     D_u = sum_{i, i'} w[k, i] w[k', i'] (M_u - M_0)[i, i']
 * for u = {l} in columns l = 0 .. d - 1 (first-order), u = all but l in columns d .. 2 d - 1, u = all inputs in column 2 d: the
 * covariance over the box, under the uniform measure, of the conditional means of ghat_k and ghat_k' given the inputs in u.
 * Column 2 d + 1: the box mean sum_i w[k, i] prod_l a_l[i] of component k in the rows with k = k', 0 elsewhere.
 * The difference M_u - M_0 is taken per element; no subset product is formed by a division.  J for two different length scales
 * comes without a division by their difference (the recipe is in DESIGN.md 4.22 and above sobol_moments in the source).
 * Always float64; the factorisation workspace is not touched.  x, w, ell, box, scratch and out are device pointers, pairs is a
 * HOST array.  Three launches per batch of 64 pairs (the table of the a_l and the means once per call): 64 x 64 tiles of the
 * (i, i') plane, a pair k = k' over the lower tiles only; the tile sums go through the scratch and are added in a fixed order:
 * no atomics, two calls agree bit for bit and nothing depends on the scratch content on entry.  d <= 16: d pair integrals per
 * element; beyond: d^2.
 * scratch: lcgp_sobol_scratch_bytes(n, d, q_all, npairs) = 8 (q_all d n + q_all + min(npairs, 64) ceil(n / 64)^2 (2 d + 1)). */
int lcgp_sobol_scratch_bytes(int n, int d, int q_all, int npairs, size_t* bytes /*host out*/);
int lcgp_sobol_pairs(void* stream, int kernel_id, int n, int d, int q_all,
                     const double* x /* n x d, standardised */, const double* w /* q_all x n */,
                     const double* ell /* q_all x d */, const double* box /* lo[d], hi[d] */,
                     const int* pairs /* npairs x 2, host */, int npairs, void* scratch,
                     double* out /* npairs x (2 d + 2) */);

/* The same pass weighted by a matrix: what the posterior uncertainty of the emulator adds to the Sobol variances, and the
 * exact box-integrated posterior variance.  For each LOCAL component k in `ks` of a float64 workspace whose
 * A^-1 slot is filled (what lcgp_fetch_matrix(which = 2) reads), with
 *     Q[i, i'] = v[k, i] v[k, i'] A_k^-1[i, i'],      v[k, i] = c_k sr_i sqrt(D_k),  c_k = scale_k (1 - nt_k)
 * and a_l, J_l, M_u, M_0 of lcgp_sobol_pairs for the pair (k, k), row r of `out` holds for k = ks[r]
 *     sum_{i, i'} Q[i, i'] (M_u - M_0)[i, i']   in columns 0 .. 2 d (u = {l}, all but l, all inputs), and
 *     S0 = sum_{i, i'} Q[i, i'] M_0[i, i']      in column 2 d + 1.
 * A^-1 is read IN PLACE, tile by tile (no n x n copy); only its lower triangle is read: the tiles with column tile <= row tile,
 * the strictly lower ones counted twice, and in a diagonal tile an element above the diagonal takes the mirrored entry.  The
 * element loop, its pair integrals and the order of every sum are those of lcgp_sobol_pairs, whose results do not change.
 * v and ell are (q_local, n) and (q_local, d), rows of the LOCAL components; x, v, ell, box, workspace, scratch and out are
 * device pointers, ks is a HOST array.  float64 only (a float32 workspace is refused), d <= 126, n >= 1, nks >= 1.  No atomics:
 * two calls agree bit for bit and nothing depends on the scratch content on entry.
 * scratch: lcgp_sobol_matrix_scratch_bytes(n, d, q_local, nks) = 8 (q_local d n + q_local + min(nks, 64) ceil(n / 64)^2 (2 d + 2)). */
int lcgp_sobol_matrix_scratch_bytes(int n, int d, int q_local, int nks, size_t* bytes /*host out*/);
int lcgp_sobol_matrix_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                            const double* x /* n x d, standardised */, const double* v /* q_local x n */,
                            const double* ell /* q_local x d */, const double* box /* lo[d], hi[d] */,
                            const void* workspace, const int* ks /* nks, host */, int nks, void* scratch,
                            double* out /* nks x (2 d + 2) */);

/* The matrix-weighted pass on a conditioned view: lcgp_sobol_matrix_pairs over the N = n + m centres
 * xa = [x; xn] (training inputs first, then the view's m inputs) with the covariance correction of the view in A^-1's place.  For
 * each LOCAL component k in `ks`, with W = L^-1 and A^-1 of the float64 workspace, U_n and L_S^-1 of the view's float64 state
 * (lcgp_condition_prepare) and D_k from the theta rows, the weight of an element is
 *     Q'[i, i'] = v[k, i] v[k, i'] (E[i, i'] + D_k A_k^-1[i, i'] [i < n and i' < n]),
 *     E = Pt^T Pt,     Pt = [ -D_k T_n W | L_S^-1 ]  (m x N),     T_n = L_S^-1 U_n,
 * the block inverse of the augmented matrix with the Schur complement S.  The split of D: D_k sits INSIDE the matrices (on A^-1
 * and on the first block of Pt); v carries the rest, v[k, i] = c_k sr_i on the n training rows and c_k on the m new rows
 * (c_k = scale_k (1 - nt_k)) -- unlike lcgp_sobol_matrix_pairs, whose v holds sqrt(D_k).  Row r of `out` is laid out as there:
 * sum Q' (M_u - M_0) in columns 0 .. 2 d, S0 = sum Q' M_0 in column 2 d + 1, M over the N centres.
 * One component at a time: -T_n and (-T_n) W on the tile kernel (OP_COND_U on a zeroed slab, OP_PRED_V), one transposing
 * launch that scales and places the L_S^-T block (zeros on all padding), the lower 64 x 64 tiles of E (OP_PRED_COV, K = mpad),
 * then ONE pair pass over the N x N plane whose tile weights are E plus, where both indices are below n, D_k A^-1 read in place.
 * The workspace, the state and theta are only read.  float64 only (a float32 workspace or state is refused), d <= 126, n >= 1,
 * m >= 1, nks >= 1; every argument is checked before the first launch.  No atomics, one stream: two calls agree bit for bit,
 * nothing depends on the scratch content on entry or on which subset of ks is asked for.  xa (N x d), v (q_local x N), ell
 * (q_local x d), box, theta, workspace, state, scratch and out are device pointers, ks is a HOST array.
 * scratch: lcgp_condition_sobol_scratch_bytes(n, d, q_local, m, nks): the table (q_local d N doubles), the tile sums of one
 * component, 2 mpad npad + Npad mpad + Npad^2 doubles for T_n, T_n W, P and E (Npad = N rounded up to 64), each 256-byte aligned. */
int lcgp_condition_sobol_scratch_bytes(int n, int d, int q_local, int m, int nks, size_t* bytes /*host out*/);
int lcgp_condition_sobol_matrix_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                      const double* theta, const void* workspace, const void* state, int m,
                                      const double* xa /* (n + m) x d, standardised */, const double* v /* q_local x (n + m) */,
                                      const double* ell /* q_local x d */, const double* box /* lo[d], hi[d] */,
                                      const int* ks /* nks, host */, int nks, void* scratch, size_t scratch_bytes,
                                      double* out /* nks x (2 d + 2) */);

/* Closed variances of a caller's list of input subsets: the pair sums of lcgp_sobol_pairs, of
 * lcgp_sobol_matrix_pairs and of lcgp_condition_sobol_matrix_pairs for ANY subsets u of the inputs instead of the 2 d + 1 fixed
 * ones -- what second-order indices, indices of groups of inputs and Shapley effects are made of.  A subset is a bit mask: bit l
 * of masks[s] is set when input l is in u; the empty mask and the full mask are allowed, a mask may repeat.  With a_l, J_l and
 *     M_u[i, i'] = prod_l (bit_l ? J_l[i, i'] : a_l[i] a'_l[i']),   l ascending   (a select per factor, never a division)
 * of lcgp_sobol_pairs, column s of a row of `out` holds for u = masks[s]
 *     lcgp_sobol_subset_pairs                    D_u = sum_{i, i'} w[k, i] w[k', i'] (M_u - M_0)[i, i']     (k, k') = pairs[r]
 *     lcgp_sobol_matrix_subset_pairs             sum_{i, i'} Q[i, i'] (M_u - M_0)[i, i']                     k = ks[r], Q as there
 *     lcgp_condition_sobol_matrix_subset_pairs   sum_{i, i'} Q'[i, i'] (M_u - M_0)[i, i']  over N = n + m centres, Q' as there
 * with M_0 the same product for the empty mask, so that the empty mask gives exactly 0.0.  The other arguments, their checks, the
 * tiles (a pair k = k' over the lower ones, the strictly lower ones twice), the element loop, the pair integrals and the
 * preparation launches are those of the three functions above, whose results do not change; no row carries a box mean or S0.
 * The expensive part of an element, its d pair integrals, does not depend on u: one launch accumulates
 * lcgp_sobol_subset_chunk(d) masks over them (32 for every d <= 16), and more masks are further launches that form the
 * integrals again: ceil(nsub / chunk) pair launches and as many reductions per batch of 64 pairs.  The tile sums go through the
 * scratch and are added in a fixed order: no atomics, two calls agree bit for bit, nothing depends on the scratch content on
 * entry, and the sum of a mask depends neither on the other masks of the call nor on its place among them.
 * Refused before the first launch (lcgp_last_error says why): NULL pointers, d > 16 (no wider variant: use the functions above
 * for the fixed subsets), a mask with a bit at or above d, nsub < 1, n < 1, and a float32 workspace for the matrix forms.
 * masks is a HOST array.  lcgp_sobol_subset_chunk returns the chunk, or a negative value for d outside [1, 16].
 * scratch: lcgp_sobol_subset_scratch_bytes(n, d, q_all, npairs, nsub) =
 *     8 (q_all d n + q_all + min(npairs, 64) ceil(n / 64)^2 chunk(d))
 * for both lcgp_sobol_subset_pairs and lcgp_sobol_matrix_subset_pairs (q_all = q_local, npairs = nks there); it does not grow
 * with nsub.  The table of the a_l comes first, then the q_all box means sum_i w[k, i] prod_l a_l[i] of the components, which a
 * caller may read there after the call, then the tile sums of one launch.
 * lcgp_condition_sobol_subset_scratch_bytes(n, d, q_local, m, nks, nsub): the layout of lcgp_condition_sobol_scratch_bytes with
 * ceil(N / 64)^2 chunk(d) tile sums in the place of its ceil(N / 64)^2 (2 d + 2). */
int lcgp_sobol_subset_chunk(int d);
int lcgp_sobol_subset_scratch_bytes(int n, int d, int q_all, int npairs, int nsub, size_t* bytes /*host out*/);
int lcgp_sobol_subset_pairs(void* stream, int kernel_id, int n, int d, int q_all,
                            const double* x /* n x d, standardised */, const double* w /* q_all x n */,
                            const double* ell /* q_all x d */, const double* box /* lo[d], hi[d] */,
                            const int* pairs /* npairs x 2, host */, int npairs,
                            const uint64_t* masks /* nsub, host */, int nsub, void* scratch,
                            double* out /* npairs x nsub */);
int lcgp_sobol_matrix_subset_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                   const double* x /* n x d, standardised */, const double* v /* q_local x n */,
                                   const double* ell /* q_local x d */, const double* box /* lo[d], hi[d] */,
                                   const void* workspace, const int* ks /* nks, host */, int nks,
                                   const uint64_t* masks /* nsub, host */, int nsub, void* scratch,
                                   double* out /* nks x nsub */);
int lcgp_condition_sobol_subset_scratch_bytes(int n, int d, int q_local, int m, int nks, int nsub, size_t* bytes /*host out*/);
int lcgp_condition_sobol_matrix_subset_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                             const double* theta, const void* workspace, const void* state, int m,
                                             const double* xa /* (n + m) x d, standardised */,
                                             const double* v /* q_local x (n + m) */, const double* ell /* q_local x d */,
                                             const double* box /* lo[d], hi[d] */, const int* ks /* nks, host */, int nks,
                                             const uint64_t* masks /* nsub, host */, int nsub, void* scratch,
                                             size_t scratch_bytes, double* out /* nks x nsub */);

/* Exact box ALC (no counterpart in the reference): for every candidate, how much the box-integrated posterior
 * variance IV_k of lcgp_sobol_matrix_pairs would drop if the simulator ran `replicates` more times there, at fixed parameters --
 * lcgp_variance_reduction with the weighted sum over a reference set replaced by the exact integral over `box` (uniform measure).
 * float64 only.  Runs behind lcgp_nll_grad at the same theta and only READS its workspace.  Per local component k, standardised
 * inputs, c = scale (1 - nt), X_c the candidate's cross-covariance row as lcgp_variance_reduction forms it (`match`: per candidate
 * the training input it replicates, whose column carries the nugget term, or -1; NULL = none; a DEVICE array), V_c = X_c A^-1,
 * b_c = D c sr o V_c, J_l the pair average of lcgp_sobol_pairs with both length scales ell_kl:
 *     M[i, i'] = prod_l J_l(x_il, x_i'l)        m_c[i] = prod_l J_l(x_cl, x_il)        m_cc = prod_l J_l(x_cl, x_cl)
 *     R_k(c) = [ c^2 m_cc - 2 c b_c . m_c + b_c^T M b_c ] / (max(scale - D |U_c|^2, 0) + 1 / (D replicates))
 * = IV_k before minus IV_k after the runs.  The three terms cancel: their absolute sum is tens to hundreds of c where R is 1e-5
 * to 1e-3 of c, so R carries an ABSOLUTE error of a few ulps of that sum; it is not clamped and may come out slightly negative
 * where the gain is at rounding level.  Candidates may lie outside the box.
 * The call handles the components k0 .. k0 + q_group - 1 of the workspace (carved for q_local) and writes their rows of `out`
 * (q_local rows of n_cand, `out_stride` apart, 0 = n_cand): a caller bounds the scratch by processing the local components in
 * groups and the candidates in chunks.  form_m != 0: (sr sr^T) o M of the group's components is materialised at the head of the
 * scratch first (box_matrix_kernel: 64 x 64 tiles with column tile <= row tile, written with their mirror, zero on the padding);
 * form_m = 0: the scratch still holds it from the preceding call with the same k0, q_group and box -- the place of M does not
 * depend on n_cand, so the chunks of one candidate set share it.
 * Launches behind it: X, U = X W^T, gvar and V = U W by the launches of lcgp_predict_grad; T = V M on the fp64 MFMA tile kernel
 * (OP_HESS_G, 128 x 128 tiles); one wave per candidate for T_c . V_c; box_cross_kernel, one workgroup per (candidate, component),
 * which forms m_c[i] in registers, sums sr_i V_ci m_c[i] over the row and combines.  Nothing of size n_cand x n x d and no
 * n_cand x n array of integrals is written.  V is formed on 64-row tiles below 128 candidates and on 128-row tiles from 128 on
 * (the two sum in different orders): a caller that wants results independent of its chunking never passes fewer than 128
 * candidates while it has them.  Every sum has a fixed order, no atomics: bitwise reproducible, independent of q_local, of k0 /
 * q_group and of the scratch content on entry.
 * Refused before the first launch: a float32 workspace, NULL pointers (sr and match may be NULL), d > 126, n < 1, n_cand < 1 or
 * > 65535, replicates < 1.
 * scratch: lcgp_box_alc_scratch_bytes(dtype, n, d, q_group, n_cand) = q_group (npad^2 + 2 n0pad npad + 3 n0pad) doubles (npad = n
 * and n0pad = n_cand rounded up to 128), each part rounded up to 256 bytes. */
int lcgp_box_alc_scratch_bytes(int dtype, int n, int d, int q_group, int n_cand, size_t* bytes /*host out*/);
int lcgp_box_alc(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                 const void* x, const void* sr, const double* theta, const void* workspace,
                 int k0, int q_group, const double* box /* lo[d], hi[d], standardised */,
                 int n_cand, const void* x_cand /* n_cand x d, standardised */, const int* match /* n_cand, or NULL */,
                 int replicates, int form_m, void* scratch,
                 double* out /* q_local rows of n_cand, `out_stride` apart */, int out_stride);

#ifdef __cplusplus
}
#endif
#endif /* LCGP_HIP_H */
