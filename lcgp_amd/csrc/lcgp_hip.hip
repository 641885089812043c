// lcgp_hip.hip -- gfx950 (MI355X) kernels + C ABI for the LCGP fit/predict hot path.
//
// What the reference does per L-BFGS-B evaluation (lcgp.py:635-666 / 554-630 + the gpflow tape):
// for each latent component k build C_k (covmat.py:31-55), decompose it, reduce to a scalar, and
// back-propagate.  Here, per component:  A = I + D (C o s s^T)  ->  A = L L^T (blocked Cholesky,
// 64x64 diagonal blocks in LDS, fp64 MFMA trailing updates)  ->  W = L^-1 (level-parallel TRMMs)
// ->  A^-1 = W^T W (one MFMA launch)  ->  z = A^-1 b  ->  fused contraction of
// G = s s^T o (D/2 A^-1 - z z^T/2) with dC/dtheta recomputed on the fly from x.
// All components of the rank are batched in every launch.  The library keeps no state: the launch schedule is a
// per-call argument (lcgp_sched), nothing is allocated, no stream or event is created.
//
// Layout in HBM: per component three npad x npad row-major matrices (npad = n rounded up to 128,
// the padding is the identity so every kernel works on whole 64x64 / 128x128 tiles):
//   M : A, then L (lower tiles)      W : L^-1 (lower tiles)      V : scratch, then A^-1 (lower tiles)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <type_traits>
#include <vector>

#include "../../include/lcgp_hip.h"
#include "fill_sched.h"
#include "sobol_subset.h"

#define LCGP_VERSION 610

namespace {

constexpr int TS = 64;    // tile size (rows/cols of one tile)
constexpr int KT = 16;    // k extent of one LDS stage
constexpr int DMAX = 32;  // input dimensions staged in LDS at once (the fused kernels are instantiated for 2, 4, 6, 10, 16, 32)
constexpr int DWIDE = 126; // largest input dimension (beyond 32: chunks of 32 dimensions, grad_kernel_wide; the per-tile partial
                           // sums of the gradient contraction hold d + 2 <= 128 doubles)

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

thread_local char g_err[256] = "";

inline int fail(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -2;
}
inline int bad(const char* what) {
    snprintf(g_err, sizeof(g_err), "bad argument: %s", what);
    return -1;
}

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---------------------------------------------------------------------------------------------------
// workspace carving (all offsets 256-byte aligned)
// ---------------------------------------------------------------------------------------------------
struct Ws {
    int n, npad, nb, d, p, q;
    int kern = 0;        // covariance kernel (lcgp_hip.h: LCGP_KERNEL_MATERN32 / LCGP_KERNEL_SE / LCGP_KERNEL_MATERN52)
    size_t esz;
    size_t mat;          // elements per matrix
    char* base;
    size_t off_M, off_W, off_V, off_b, off_z, off_part, off_cpart, off_c, off_logdet, off_info, off_clock, total;
    int ntile_lower;
};

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

inline Ws carve(int dtype, int n, int d, int p, int q, void* base) {
    Ws w;
    w.n = n; w.d = d; w.p = p; w.q = q;
    w.npad = round_up(n, 2 * TS);   // whole 128x128 super-tiles (identity padding)
    w.nb = w.npad / TS;
    w.esz = dtype == LCGP_F64 ? 8 : 4;
    w.mat = (size_t)w.npad * w.npad;
    w.base = (char*)base;
    w.ntile_lower = w.nb * (w.nb + 1) / 2;
    size_t o = 0;
    w.off_M = o; o = align256(o + w.mat * q * w.esz);
    w.off_W = o; o = align256(o + w.mat * q * w.esz);
    w.off_V = o; o = align256(o + w.mat * q * w.esz);
    w.off_b = o; o = align256(o + (size_t)w.npad * q * w.esz);
    w.off_z = o; o = align256(o + (size_t)w.npad * q * w.esz);
    w.off_part = o; o = align256(o + (size_t)w.ntile_lower * q * 2 * TS * sizeof(double));   // symv partials (2 x 64 per
                                                                                          // tile), then gradient partials
    // float32 only: c = (C o s s^T) z in double (per-tile partials, then the vector), see grad_kernel
    w.off_cpart = o; o = align256(o + (dtype == LCGP_F64 ? 0 : (size_t)w.ntile_lower * q * 2 * TS * sizeof(double)));
    w.off_c = o; o = align256(o + (dtype == LCGP_F64 ? 0 : (size_t)w.npad * q * sizeof(double)));
    w.off_logdet = o; o = align256(o + (size_t)q * sizeof(double));
    w.off_info = o; o = align256(o + (size_t)q * sizeof(int));
    w.off_clock = o; o = align256(o + 4 * sizeof(unsigned long long));     // shader-clock / real-time stamps of the last A^-1 launch
    w.total = o;
    return w;
}

// ---------------------------------------------------------------------------------------------------
// MFMA wrappers.  A/B operand: lane l holds A[i = l & 15][k = l >> 4] / B[k = l >> 4][j = l & 15].
// C/D: col = l & 15;  row = (l >> 4) + 4 * reg for f64,  (l >> 4) * 4 + reg for f32.
// ---------------------------------------------------------------------------------------------------
template <typename T> struct Mfma;
template <> struct Mfma<double> {
    typedef d4 acc_t;
    static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
    static __device__ __forceinline__ int lane_row(int lane) { return lane >> 4; }      // row = lane_row + reg_row
    static __device__ __forceinline__ constexpr int reg_row(int reg) { return 4 * reg; }
};
template <> struct Mfma<float> {
    typedef f4 acc_t;
    static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
    static __device__ __forceinline__ int lane_row(int lane) { return (lane >> 4) * 4; }
    static __device__ __forceinline__ constexpr int reg_row(int reg) { return reg; }
};

// Buffer addressing of a tile: descriptor (base pointer, in scalar registers) + scalar byte offset + one per-lane byte
// offset register + immediate.  An accumulator tile addressed through 64-bit per-lane pointers costs two registers per
// distinct row of the MFMA lane map (16 of the 128 a wave of the fp64 128-tile kernels may use), held across the K loop.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
template <typename T> struct BufIo;
template <> struct BufIo<double> {
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ double load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
    }
    static __device__ __forceinline__ void store(double v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, voff, soff, 0);
    }
};
template <> struct BufIo<float> {
    static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
    }
    static __device__ __forceinline__ void store(float v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
    }
};

// Thread index of a tile body.  Opaque to the optimiser on purpose: where bodies sit in a loop (the chain workgroup of
// host_kernel), every lane-dependent address computation of every body would otherwise be hoisted in front of that loop
// and kept alive across it (the diagonal-block code needs the whole register file itself).
__device__ __forceinline__ int body_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    __builtin_assume(t >= 0 && t < 1024);
    return t;
}

__device__ __forceinline__ void tri_decode(int t, int& r, int& c) {
    int rr = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((rr + 1) * (rr + 2) / 2 <= t) ++rr;
    while (rr * (rr + 1) / 2 > t) --rr;
    r = rr;
    c = t - rr * (rr + 1) / 2;
}

// theta block accessors
__device__ __forceinline__ const double* th_row(const double* theta, int d, int p, int k) {
    return theta + (size_t)k * (d + 3 + p);
}

// exp(x) for x <= 0 (the kernel's -sum_j S_j): Cody-Waite reduction x = k ln2 + r, degree-13 Taylor polynomial on
// |r| <= ln2/2 (truncation 4e-18), scaling by v_ldexp_f64.  <= 1 ulp against libm over [-745, 0] (20 M samples on the
// host); about half the instructions of the library exp, whose overflow / NaN handling cannot occur here -- the
// kernel build and the gradient contraction are bound by fp64 VALU issue, not by HBM, with the library version.
// p * r + c with the constant c held in a SCALAR register pair: as a literal the compiler re-materialises every 64-bit
// constant with two v_mov per use (a quarter of the kernel-build instructions, which is bound by VALU issue)
__device__ __forceinline__ double fma_sc(double p, double r, double c) {
    double o;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(o) : "v"(p), "v"(r), "s"(c));
    return o;
}

__device__ __forceinline__ double exp_nonpos(double x) {
    const double kf = rint(x * 1.4426950408889634074);
    double r = fma(-kf, 6.93147180369123816490e-01, x);
    r = fma(-kf, 1.90821492927058770002e-10, r);
    double p = fma_sc(1.6059043836821613e-10, r, 2.08767569878681e-09);     // 1/13!, 1/12!
    p = fma_sc(p, r, 2.505210838544172e-08);
    p = fma_sc(p, r, 2.755731922398589e-07);
    p = fma_sc(p, r, 2.7557319223985893e-06);
    p = fma_sc(p, r, 2.48015873015873e-05);
    p = fma_sc(p, r, 1.984126984126984e-04);
    p = fma_sc(p, r, 1.388888888888889e-03);
    p = fma_sc(p, r, 8.333333333333333e-03);
    p = fma_sc(p, r, 4.1666666666666664e-02);
    p = fma_sc(p, r, 1.6666666666666666e-01);
    p = fma_sc(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)kf);
}
// float32 (no reference precision to match): v_exp_f32 on x log2(e); the absolute error stays below 1e-7
__device__ __forceinline__ float exp_nonpos(float x) { return __expf(x); }

// C0 = prod_j (1 + S_j) exp(-sum_j S_j): where the exponent is below the smallest normal number's logarithm the value is
// zero for every purpose of the path -- but the POLYNOMIAL there may have overflowed (lengthscales at their lower SoftClip
// bound 1e-6: S_j ~ 1e6, ten dimensions: 1e60, beyond float32's range), and inf x 0 is a NaN that takes the whole
// factorisation with it: this is what ended float32 fits of configs[3] (profiles/r06_fp32_breakdown.txt: status word 2 at
// lambda_max(A) ~ 5 .. 130, i.e. nothing to do with conditioning).  Above the threshold prod (1 + S_j) <= exp(sum S_j) is
// finite.  The matrices stay identical wherever they were finite before.
// (kernel build / cross covariance: the polynomial is capped instead -- one v_min per element in a kernel bound by VALU issue;
// prod (1 + S_j) <= exp(sum S_j), so a polynomial beyond the cap meets an exponential that has underflowed to zero long before)
template <typename T> __device__ __forceinline__ constexpr T poly_cap();
template <> __device__ __forceinline__ constexpr double poly_cap<double>() { return 1e300; }
template <> __device__ __forceinline__ constexpr float poly_cap<float>() { return 1e38f; }
template <typename T> __device__ __forceinline__ constexpr T exp_floor();
template <> __device__ __forceinline__ constexpr double exp_floor<double>() { return -708.0; }
template <> __device__ __forceinline__ constexpr float exp_floor<float>() { return -87.0f; }

// Covariance kernel ids (lcgp_hip.h): every device function templated on KERN spells out all three; a site that only
// told "0" from "not 0" would silently evaluate the squared exponential for a new id.
template <int KERN> struct kern_known { static constexpr bool value = KERN == 0 || KERN == 1 || KERN == 2; };
// Matern-5/2 (KERN == 2), the reference's Matern-3/2 convention carried over (no sqrt(5)): per dimension the factor
//   f(S) = 1 + S + S^2 / 3   beside exp(-S),     C0 = prod_j f(S_j) exp(-sum_j S_j),
// i.e. the textbook Matern-5/2 at lengthscale sqrt(5) ell_j.  f(S) <= exp(S), so the guards of the 3/2 path carry over
// unchanged: a product beyond poly_cap (or inf, or the NaN of inf x 0 -- fmin returns its other operand) meets an
// exponential that has underflowed to zero.  m52_fm1 = f - 1 (the form `poly = fma(poly, f - 1, poly)` of the 3/2 path);
//   dC0/d ell_j  = C0 m52_wl(S_j) / (f(S_j) ell_j),     m52_wl(S) = S^2 (1 + S) / 3
//   dC0/d x1_j   = -C0 m52_wx(s_j) / ell_j,             m52_wx(s) = s (1 + |s|) / (3 + 3 |s| + s^2)  (|m52_wx| < 1)
template <typename T> __device__ __forceinline__ T m52_fm1(T sd) { return fma(sd * (T)(1.0 / 3.0), sd, sd); }
__device__ __forceinline__ double m52_wl(double sd) { return (sd * sd) * fma(sd, 1.0 / 3.0, 1.0 / 3.0); }
// the value of the product kernel from its two accumulated parts (SE carries no polynomial)
template <int KERN>
__device__ __forceinline__ double kern_c0(double poly, double ssum) {
    static_assert(kern_known<KERN>::value, "unknown covariance kernel id");
    if constexpr (KERN == 1) return exp_nonpos(ssum);
    else return fmin(poly, poly_cap<double>()) * exp_nonpos(ssum);
}

// ---------------------------------------------------------------------------------------------------
// K1: kernel build.   A_ij = delta_ij + D sr_i sr_j s ((1 - nt) C0_ij + nt delta_ij)
//   C0 = prod_j (1 + S_j) exp(-sum_j S_j),  S_j = |x_i,j/ell_j - x_i',j/ell_j|      (covmat.py:35-53)
// One 64x64 lower tile per workgroup; x rows/cols staged in LDS already divided by ell.
// ---------------------------------------------------------------------------------------------------
// KERN: 0 = the reference's separable Matern-3/2 product (covmat.py:31-55), 1 = squared-exponential product kernel
//   C0 = exp(-1/2 sum_j S_j^2)   (no counterpart in the reference: BASELINE.json's north star names it; parity unpinned)
template <typename T, int DD /* >= d: the per-dimension loop is unrolled to DD */, int KERN>
__global__ __launch_bounds__(256) void build_kernel(T* __restrict__ M, size_t mat, int n, int npad, int d, int p,
                                                    const T* __restrict__ x, const T* __restrict__ sr,
                                                    const double* __restrict__ theta, int ntile,
                                                    const T* __restrict__ Y, T* __restrict__ bvec,
                                                    double* __restrict__ logdet, int* __restrict__ info) {
    // arithmetic in the storage type: the float32 variant is the HBM-bound regime (one float exp per element)
    __shared__ T xr[TS][DD + 1];
    __shared__ T xc[TS][DD + 1];
    __shared__ T srr[TS], src[TS];
    const int k = blockIdx.y;
    if ((int)blockIdx.x >= ntile) {
        // blocks past the tiles: b_k[i] = sum_a Y[a, i] psi_k[a]  (lcgp.py:646 + 657-658 collapsed; 608-610 for rep),
        // independent of the matrix, so it rides in this launch instead of a launch of its own
        const int i = (blockIdx.x - ntile) * 256 + threadIdx.x;
        if (i == 0 && logdet) { logdet[k] = 0.0; info[k] = 0; }      // the factorisation that follows starts from zero
        if (i >= npad) return;
        const double* psi = th_row(theta, d, p, k) + d + 3;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (i < n) {
            int a = 0;
            for (; a + 3 < p; a += 4) {
                s0 += (double)Y[(size_t)a * n + i] * psi[a];
                s1 += (double)Y[(size_t)(a + 1) * n + i] * psi[a + 1];
                s2 += (double)Y[(size_t)(a + 2) * n + i] * psi[a + 2];
                s3 += (double)Y[(size_t)(a + 3) * n + i] * psi[a + 3];
            }
            for (; a < p; ++a) s0 += (double)Y[(size_t)a * n + i] * psi[a];
        }
        bvec[(size_t)k * npad + i] = (T)((s0 + s1) + (s2 + s3));
        return;
    }
    int r, c;
    tri_decode(blockIdx.x, r, c);
    const double* th = th_row(theta, d, p, k);
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double nt = nug / (1.0 + nug);
    const T c_off = (T)(D * scale * (1.0 - nt));        // multiplies C0
    const T c_diag = (T)(1.0 + D * scale * nt);         // extra term on the diagonal (times sr_i^2)
    const int tid = threadIdx.x;
    if (tid < TS) {
        int gi = r * TS + tid, gj = c * TS + tid;
        srr[tid] = (sr && gi < n) ? sr[gi] : (T)1;
        src[tid] = (sr && gj < n) ? sr[gj] : (T)1;
    }
    T* Mk = M + (size_t)k * mat;
    // 4 x 4 elements per thread (16 x 16 threads per tile): every LDS read of a scaled input row/column is used four
    // times, 16 independent exp chains per thread.  Columns per thread: in fp32 four consecutive ones (one 16-byte store
    // per row; the 16 lanes of a row write 256 contiguous bytes); in fp64 the pairs {2 tx, 2 tx + 1} and {32 + 2 tx, 33 + 2 tx},
    // so that EACH 16-byte store instruction of the 16 lanes covers 256 contiguous bytes (with four consecutive columns
    // per thread every instruction would write 16 of each 32 bytes: two partial passes over every line)
    const int tx = tid & 15, ty = tid >> 4;
    const int i0 = ty * 4;
    constexpr bool PAIRS = sizeof(T) == 8;
    auto colof = [&](int b) { return PAIRS ? (b >> 1) * 32 + 2 * tx + (b & 1) : 4 * tx + b; };
    T poly[4][4], ssum[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { poly[a][b] = (T)1; ssum[a][b] = (T)0; }
    constexpr int UNR = DD <= 6 ? DD : 2;          // (fully unrolled the LDS reads of all dimensions are hoisted: registers)
    // one chunk of (at most) DD dimensions starting at d0: staged in LDS divided by ell, then accumulated
    auto chunk = [&](const int d0) {
        for (int e = tid; e < TS * DD; e += 256) {         // (columns beyond d are zero: they add |0 - 0| = 0)
            int i = e / DD, j = e - i * DD;
            int gi = r * TS + i, gj = c * TS + i;
            xr[i][j] = (gi < n && d0 + j < d) ? (T)((double)x[(size_t)gi * d + d0 + j] / th[d0 + j]) : (T)0;
            xc[i][j] = (gj < n && d0 + j < d) ? (T)((double)x[(size_t)gj * d + d0 + j] / th[d0 + j]) : (T)0;
        }
        __syncthreads();
#pragma unroll UNR
        for (int jj = 0; jj < DD; ++jj) {
            T xa[4], xb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { xa[a] = xr[i0 + a][jj]; xb[a] = xc[colof(a)][jj]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if constexpr (KERN == 0) {
                        const T sd = fabs(xa[a] - xb[b]);
                        poly[a][b] = fma(poly[a][b], sd, poly[a][b]);
                        ssum[a][b] -= sd;
                    } else if constexpr (KERN == 1) {
                        const T df = xa[a] - xb[b];
                        ssum[a][b] = fma((T)-0.5 * df, df, ssum[a][b]);
                    } else {
                        static_assert(KERN == 2, "unknown covariance kernel id");
                        const T sd = fabs(xa[a] - xb[b]);
                        poly[a][b] = fma(poly[a][b], m52_fm1(sd), poly[a][b]);
                        ssum[a][b] -= sd;
                    }
                }
        }
    };
    if constexpr (DD == DMAX) {
        // the widest instantiation also serves d > 32 (covmat.py:35-42 loops over any d): 32 dimensions at a time
        for (int d0 = 0; d0 < d; d0 += DD) {
            if (d0 > 0) __syncthreads();
            chunk(d0);
        }
    } else {
        chunk(0);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int gi = r * TS + i0 + a;
        T v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int gj = c * TS + colof(b);
            if (gi < n && gj < n) {
                const T c0 = fmin(poly[a][b], poly_cap<T>()) * exp_nonpos(ssum[a][b]);
                const T ss = srr[i0 + a] * src[colof(b)];
                v[b] = ss * c_off * c0;
                if (gi == gj) v[b] += (T)1 + (c_diag - (T)1) * ss;
            } else {
                v[b] = gi == gj ? (T)1 : (T)0;
            }
        }
        T* dst = Mk + (size_t)gi * npad + c * TS;
        if constexpr (PAIRS) {
            typedef T pair_t __attribute__((ext_vector_type(2)));
            *(pair_t*)(dst + colof(0)) = pair_t{v[0], v[1]};
            *(pair_t*)(dst + colof(2)) = pair_t{v[2], v[3]};
        } else {
            typedef T quad_t __attribute__((ext_vector_type(4)));
            *(quad_t*)(dst + colof(0)) = quad_t{v[0], v[1], v[2], v[3]};
        }
    }
}

// rectangular Matern32 (covmat.py:31-55): out (n1 x n2) = scale ((1-nt) C0 + nt I[same]) o colscale^T.
// Parameters come either by value (host call, lcgp_matern32) or from a device theta row (predict).
struct ThetaArg { double v[DWIDE + 2]; };

// MARG (lcgp_predict_marginal; the instances with the two extra arguments mask and tab): row i of x1 carries a mask of
// INTEGRATED dimensions (mask[i d + l] != 0, n1 x d bytes).  Such a dimension's entry of x1 is never loaded; its factor is
// the box average of the 1-D kernel factor at the training input, read from the table tab[(k d + l) n2pad + j]
// (marg_table_kernel) and multiplied into poly; ssum is left alone.  Rows with an empty mask go through exactly the operations
// of the plain kernel.  Every MARG statement sits behind `if constexpr`, and the plain instances have an empty pack: the
// signature and the code lcgp_predict and the others launch are those of the kernel without the variant.
__device__ __forceinline__ void marg_args(const unsigned char*& mask, const double*& tab, const unsigned char* m, const double* t) {
    mask = m;
    tab = t;
}

template <typename T, int KERN, typename... EX>
__global__ __launch_bounds__(256) void cross_kernel(T* __restrict__ out, int ldo, int n1, int n2, int d,
                                                    const T* __restrict__ x1, const T* __restrict__ x2,
                                                    ThetaArg tv, const double* __restrict__ thp /*ell[d], scale, nug*/,
                                                    int same, const T* __restrict__ colscale, int n1pad, int n2pad,
                                                    int th_stride /*doubles between the theta rows of components*/,
                                                    size_t out_stride /*elements between the output slabs*/,
                                                    const int* __restrict__ match /*per row of x1: the column of its nugget
                                                                                    term, -1 = none; NULL: `same` decides*/,
                                                    EX... ex /*MARG: const unsigned char* mask, const double* tab*/) {
    constexpr bool MARG = sizeof...(EX) != 0;
    const unsigned char* mask = nullptr;
    const double* tab = nullptr;
    if constexpr (MARG) marg_args(mask, tab, ex...);
    __shared__ double xr[TS][DMAX + 1];
    __shared__ double xc[TS][DMAX + 1];
    __shared__ double cs[TS];
    __shared__ double th[DWIDE + 2];
    __shared__ double tb[MARG ? DMAX : 1][MARG ? TS : 1];            // the table's entries of this chunk and column tile
    __shared__ unsigned char mr[MARG ? TS : 1][MARG ? DMAX : 1];     // the masks of this row tile, this chunk
    const int r = blockIdx.y, c = blockIdx.x;
    const int tid = threadIdx.x;
    if (thp) thp += (size_t)blockIdx.z * th_stride;
    out += (size_t)blockIdx.z * out_stride;
    if (tid < d + 2) th[tid] = thp ? thp[tid] : tv.v[tid];
    if (tid < TS) {
        int gj = c * TS + tid;
        cs[tid] = (colscale && gj < n2) ? (double)colscale[gj] : 1.0;
    }
    __syncthreads();
    const double scale = th[d], nug = th[d + 1];
    const double nt = nug / (1.0 + nug);
    const int j = tid & 63;
    const int gj = c * TS + j;
    double poly[16], ssum[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) { poly[m] = 1.0; ssum[m] = 0.0; }
    for (int d0 = 0; d0 < d; d0 += DMAX) {           // the dimensions in chunks of 32 (covmat.py:35-42 loops over any d)
        const int dc = d - d0 < DMAX ? d - d0 : DMAX;
        if (d0 > 0) __syncthreads();
        for (int e = tid; e < TS * dc; e += 256) {
            int i = e / dc, jj = e - i * dc;
            int gi = r * TS + i, gjj = c * TS + i;
            if constexpr (MARG) {
                const bool mk = gi < n1 && mask[(size_t)gi * d + d0 + jj] != 0;
                mr[i][jj] = mk;
                xr[i][jj] = (gi < n1 && !mk) ? (double)x1[(size_t)gi * d + d0 + jj] / th[d0 + jj] : 0.0;
            } else {
                xr[i][jj] = gi < n1 ? (double)x1[(size_t)gi * d + d0 + jj] / th[d0 + jj] : 0.0;
            }
            xc[i][jj] = gjj < n2 ? (double)x2[(size_t)gjj * d + d0 + jj] / th[d0 + jj] : 0.0;
        }
        if constexpr (MARG) {
            for (int e = tid; e < TS * dc; e += 256) {       // (c TS + t < n2pad: the grid has n2pad / TS column tiles)
                const int jj = e / TS, t = e - jj * TS;
                tb[jj][t] = tab[((size_t)blockIdx.z * d + d0 + jj) * n2pad + c * TS + t];
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int i = (tid >> 6) * 16 + m;
            for (int jj = 0; jj < dc; ++jj) {
                if constexpr (MARG) {
                    if (mr[i][jj]) { poly[m] *= tb[jj][j]; continue; }      // (uniform over the wave: i is)
                }
                if constexpr (KERN == 0) {
                    double sd = fabs(xr[i][jj] - xc[j][jj]);
                    poly[m] *= 1.0 + sd;
                    ssum[m] -= sd;
                } else if constexpr (KERN == 1) {
                    const double df = xr[i][jj] - xc[j][jj];
                    ssum[m] = fma(-0.5 * df, df, ssum[m]);
                } else {
                    static_assert(KERN == 2, "unknown covariance kernel id");
                    const double sd = fabs(xr[i][jj] - xc[j][jj]);
                    poly[m] = fma(poly[m], m52_fm1(sd), poly[m]);
                    ssum[m] -= sd;
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int i = (tid >> 6) * 16 + m;
        const int gi = r * TS + i;
        if (gi >= n1pad || gj >= n2pad) continue;
        double v = 0.0;
        if (gi < n1 && gj < n2) {
            double c0 = fmin(poly[m], poly_cap<double>()) * exp_nonpos(ssum[m]);
            // same = 1 + row offset of x1 within x2; match: row gi is training input match[gi] (a replicate of it)
            const bool on = match ? match[gi] == gj : (same && gi + (same - 1) == gj);
            double dl = on ? 1.0 : 0.0;
            v = scale * ((1.0 - nt) * c0 + nt * dl) * cs[j];
        }
        out[(size_t)gi * ldo + gj] = (T)v;
    }
}

// ---------------------------------------------------------------------------------------------------
// Box averages of the 1-D kernel factors (lcgp_predict_marginal).  kappa(u), u = |t - x| / ell:  (1 + u) e^-u (Matern-3/2),
// e^(-u^2 / 2) (SE), (1 + u + u^2 / 3) e^-u (Matern-5/2).  F(b) = int_0^b kappa, G(b) = int_0^b u kappa(u) du, Fc(b) =
// int_b^inf kappa.  The closed forms of the Matern pair subtract O(1) terms that cancel for small b (G ~ b^2 / 2), so below
// b = 1/2 both are summed from the Taylor series of kappa, kappa(u) = sum_m f(m) (-u)^m / m! with f(m) = 1 - m (Matern-3/2)
// and (m - 1)(m - 3) / 3 (Matern-5/2): 20 terms, the first one left out is below 1e-24.  SE: erf and expm1, no cancellation.
// ---------------------------------------------------------------------------------------------------
constexpr double MARG_SERIES_BELOW = 0.5;
constexpr int MARG_SERIES_TERMS = 20;

template <int KERN>
__device__ __forceinline__ void marg_series(double b, double& F, double& G) {
    double t = 1.0, sf = 0.0, sg = 0.0;                    // t = (-b)^m / m!
    for (int m = 0; m < MARG_SERIES_TERMS; ++m) {
        const double f = KERN == 0 ? 1.0 - m : (m - 1.0) * (m - 3.0) / 3.0;
        sf += t * f / (m + 1.0);
        sg += t * f / (m + 2.0);
        t *= -b / (m + 1.0);
    }
    F = b * sf;
    G = b * b * sg;
}

template <int KERN>
__device__ __forceinline__ double marg_F(double b) {
    if constexpr (KERN == 1) {
        return 1.2533141373155003 * erf(b * 0.70710678118654752);            // sqrt(pi / 2), 1 / sqrt(2)
    } else {
        if (b < MARG_SERIES_BELOW) { double F, G; marg_series<KERN>(b, F, G); return F; }
        const double e = exp(-b), em = -expm1(-b);
        if constexpr (KERN == 0) return 2.0 * em - b * e;
        else return (8.0 / 3.0) * em - b * (5.0 + b) / 3.0 * e;
    }
}

template <int KERN>
__device__ __forceinline__ double marg_G(double b) {
    if constexpr (KERN == 1) {
        return -expm1(-0.5 * b * b);
    } else {
        if (b < MARG_SERIES_BELOW) { double F, G; marg_series<KERN>(b, F, G); return G; }
        const double e = exp(-b), em = -expm1(-b);
        if constexpr (KERN == 0) return 3.0 * em - b * (3.0 + b) * e;
        else return 5.0 * em - b * (5.0 + b * (2.0 + b / 3.0)) * e;
    }
}

template <int KERN>
__device__ __forceinline__ double marg_Fc(double b) {
    if constexpr (KERN == 0) return (2.0 + b) * exp(-b);
    else if constexpr (KERN == 1) return 1.2533141373155003 * erfc(b * 0.70710678118654752);
    else return (8.0 + b * (5.0 + b)) / 3.0 * exp(-b);
}

// (1 / w) int_lo^hi kappa(|t - xv| / ell) dt, w = hi - lo: the box average of the 1-D kernel factor at the value xv (a training
// input's in marg_table_kernel, a query row's in marg_refcov_kernel; the cases are spelt out below)
template <int KERN>
__device__ __forceinline__ double marg_I1(double xv, double lo, double hi, double ell) {
    const double w = hi - lo;
    const double a1 = xv - lo, a2 = hi - xv;
    const double b1 = fabs(a1) / ell, b2 = fabs(a2) / ell;
    double r;
    if (a1 >= 0.0 && a2 >= 0.0) {
        r = marg_F<KERN>(b1) + marg_F<KERN>(b2);
    } else {
        const double bn = fmin(b1, b2), bf = fmax(b1, b2);
        r = bn > 1.0 ? marg_Fc<KERN>(bn) - marg_Fc<KERN>(bf) : marg_F<KERN>(bf) - marg_F<KERN>(bn);
    }
    return ell / w * r;
}

// I1[k, l, j] = (1 / w_l) int_lo^hi kappa(|t - x_jl| / ell_kl) dt  for every training input (columns n .. npad - 1: 1), and
// I2[k, l] = (1 / w_l^2) int int kappa(|t - t'| / ell_kl) dt dt' = 2 [F(a) / a - G(a) / a^2], a = w_l / ell_kl.
// x inside the box: (ell / w) [F(b1) + F(b2)], b = the scaled distances to the two ends.  Outside: the difference of the two,
// taken between the tails Fc once the nearer end is more than one length scale away (F saturates there and the difference
// of two saturated values would lose the small result).  grid (npad / 256, d, q); everything in double.
template <typename T, int KERN>
__global__ __launch_bounds__(256) void marg_table_kernel(const T* __restrict__ x, int n, int npad, int d,
                                                         const double* __restrict__ theta, int tw,
                                                         const double* __restrict__ box /*lo[d], hi[d]*/,
                                                         double* __restrict__ tab, double* __restrict__ i2) {
    const int j = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, k = blockIdx.z;
    const double ell = theta[(size_t)k * tw + l];
    const double lo = box[l], hi = box[d + l], w = hi - lo;
    if (j == 0) {
        const double a = w / ell;
        i2[(size_t)k * d + l] = 2.0 * (marg_F<KERN>(a) / a - marg_G<KERN>(a) / (a * a));
    }
    if (j >= npad) return;
    double v = 1.0;
    if (j < n) {
        v = marg_I1<KERN>((double)x[(size_t)j * d + l], lo, hi, ell);
    }
    tab[((size_t)k * d + l) * npad + j] = v;
}

// ---------------------------------------------------------------------------------------------------
// K2a: diagonal block.  Factorises the 64x64 block jb of M (L written back, upper part zeroed), writes its
// inverse into W (upper part zero), adds sum log L_ii to logdet[k], records info[k].  One workgroup per
// component.  The block lives in REGISTERS (thread (cj, rg) owns rows rg, rg+4, .. of column cj); per pivot
// the un-scaled pivot column goes through a double-buffered 64-entry LDS line, so the 64-step chain costs one
// barrier per step, and the update uses a_ij -= c_i (c_j / c_ss) so no sqrt sits on the chain.  The scaling
// by 1/sqrt(pivot), the log-determinant and the blocked (16) triangular inverse run after the chain.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fast_rcp(double a) {
    // v_rcp_f64 (~26 bits) + two Newton steps: full double accuracy without the IEEE division sequence
    double x = __builtin_amdgcn_rcp(a);
    x = fma(fma(-a, x, 1.0), x, x);
    x = fma(fma(-a, x, 1.0), x, x);
    return x;
}

// ---- in-wave panel factorisation of the diagonal block ----
// The 64x64 block is split into four 16-column panels, one per wave.  Wave w keeps block column w as fp64 MFMA
// accumulators (lane (c = l & 15, g = l >> 4), reg e <-> row 16 rb + g + 4 e, column 16 w + c).  When its turn
// comes it re-reads the panel through a private LDS scratch into a layout made for the 16-pivot chain:
//   lane (i = l & 15, j = l >> 4):  rD[c] = row i of the panel's 16x16 DIAGONAL block (the same in all four lane rows),
//                                   rL[c] = row i of the j-th 16x16 block BELOW it (j < 3 - kb)
// so that everything a pivot step broadcasts lives in its own 16-lane row: the update
//   a_ic -= (u_i / d) u_c        u = the un-scaled pivot column (u = l sqrt(d)), u_c held by lane c of the row
// is ONE v_fmac_f64 with the DPP modifier row_newbcast:c on u (fp64 DPP exists for exactly this control) -- no
// v_readlane pair, no SGPR hazard nop, no LDS, no barrier.  The 1/sqrt(d) scaling runs after the chain.  The finished
// panel goes to LDS as lt[col][row]; after ONE barrier the waves to its right apply it with 16x16x4 MFMAs.
// Chain per panel: 16 x (broadcast, rcp + 2 Newton steps, 2 products) with the 2 (15 - s) updates filling the shadow.
template <int C>
__device__ __forceinline__ double row_bcast(double x) {        // lane C of every 16-lane row -> the whole row
    double o;
    // s_nop 1: a DPP read needs two wait states after a VALU write of its source (x has usually just been produced)
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(x), "n"(C));
    return o;
}

template <int C>
__device__ __forceinline__ void fmac_row_bcast(double& acc, double u, double v) {   // acc += u[lane C of the row] * v
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(u), "v"(v), "n"(C));
}

template <int S, int C>
struct PivotCols {      // columns C .. 15 of pivot step S
    static __device__ __forceinline__ void run(double (&rD)[16], double (&rL)[16], double vD, double vL) {
        if constexpr (C < 16) {
            fmac_row_bcast<C>(rD[C], rD[S], vD);
            fmac_row_bcast<C>(rL[C], rD[S], vL);
            PivotCols<S, C + 1>::run(rD, rL, vD, vL);
        }
    }
};

template <int S>
struct PivotSteps {     // pivot steps S .. 15; dmine collects the pivot of row i (lane i of each row)
    static __device__ __forceinline__ void run(double (&rD)[16], double (&rL)[16], double& dmine, int i) {
        if constexpr (S < 16) {
            // rD[S] was last written by the previous step's first update: the broadcast carries the DPP wait states,
            // and every fmac of this step depends on it through vD / vL
            const double dp = row_bcast<S>(rD[S]);
            dmine = i == S ? rD[S] : dmine;
            const double rdp = fast_rcp(dp);
            const double vD = -rD[S] * rdp, vL = -rL[S] * rdp;
            PivotCols<S, S + 1>::run(rD, rL, vD, vL);
            PivotSteps<S + 1>::run(rD, rL, dmine, i);
        }
    }
};

template <int S>
struct ScaleCols {      // l = u / sqrt(pivot): column S times the reciprocal root held by lane S of the row
    static __device__ __forceinline__ void run(double (&rD)[16], double (&rL)[16], double rsl) {
        if constexpr (S < 16) {
            const double f = row_bcast<S>(rsl);
            rD[S] *= f;
            rL[S] *= f;
            ScaleCols<S + 1>::run(rD, rL, rsl);
        }
    }
};

__device__ __forceinline__ double fast_rsqrt(double a) {
    double y = __builtin_amdgcn_rsq(a);
    double e = fma(-(a * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-(a * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    return y;
}

constexpr int LEAF_LDT = TS + 1;
constexpr int LEAF_SCR = TS * 17;                                         // ONE [64][17] transposition scratch: only one wave factors at a time
constexpr int LEAF_LDS_BYTES = (2 * TS * LEAF_LDT + LEAF_SCR + 2 * TS) * 8 + 16;    // lt + w + scratch + dinv + pivs + bad

// Inverse of the lower-triangular 64x64 block, one 16-row block ROW at a time, by ONE wave (no workgroup barrier inside):
//   W_aa by substitution (lanes 0..15: one column each, solve L_aa w = e_c), then for b < a
//   T_ab = sum_{m=b}^{a-1} L_am W_mb ;  W_ab = -W_aa T_ab   on the fp64 MFMA.  The accumulator of T (lane: col = l & 15,
//   rows (l >> 4) + 4 reg) is exactly the B-operand fragment of the second product (k = 4 step + (l >> 4)).
// Needs L rows of block a and the rows < a of W: row a of the inverse can be formed as soon as panel a is factored.
__device__ __forceinline__ void leaf_inverse_diag(double (*lt)[LEAF_LDT], double (*w)[LEAF_LDT], const double* dinv, int a,
                                                  int lane) {
    if (lane < 16) {
        const int b0 = a * 16, cl = lane;
        double wc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            double sacc = i == cl ? -1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < i; ++m) sacc = fma(lt[b0 + m][b0 + i], wc[m], sacc);
            wc[i] = -sacc * dinv[b0 + i];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) w[b0 + i][b0 + cl] = wc[i];
    }
}

__device__ __forceinline__ d4 leaf_inverse_t(double (*lt)[LEAF_LDT], double (*w)[LEAF_LDT], int a, int b, int lane) {
    const int li = lane & 15, lq = lane >> 4;
    d4 tacc = {0.0, 0.0, 0.0, 0.0};
    for (int mb = b; mb < a; ++mb) {
#pragma unroll
        for (int st = 0; st < 4; ++st)
            tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(lt[mb * 16 + 4 * st + lq][a * 16 + li], w[mb * 16 + 4 * st + lq][b * 16 + li],
                                                        tacc, 0, 0, 0);
    }
    return tacc;
}

__device__ __forceinline__ void leaf_inverse_w(double (*w)[LEAF_LDT], const d4& tacc, int a, int b, int lane) {
    const int li = lane & 15, lq = lane >> 4;
    d4 wacc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int st = 0; st < 4; ++st)
        wacc = __builtin_amdgcn_mfma_f64_16x16x4f64(w[a * 16 + li][a * 16 + 4 * st + lq], tacc[st], wacc, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) w[a * 16 + lq + 4 * e][b * 16 + li] = -wacc[e];
}

// Factor AND inverse of the diagonal block.  While wave kb factors its 16-column panel (the 16-pivot chain, alone on its
// SIMD), wave kb-1 -- idle otherwise -- forms row kb-1 of the inverse from the panels that are already final; only row 3
// is left when the last panel is done, and that one is spread over all four waves.
// The results leave for memory as they become final, on waves that would otherwise wait at the panel's barrier: L panel
// kb-1 and row block kb-2 of the inverse during panel kb (and the zero quadrant beside W during panel 0), so that only
// the last panel, the last two row blocks and the log-determinant are left after the chain.
template <typename T>
__device__ __forceinline__ void leaf_store_l_panel(T* __restrict__ Mb, int npad, double (*lt)[LEAF_LDT], int pb, int lane) {
    const int col = pb * 16 + (lane & 15);
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int i = (lane >> 4) + 4 * m;
        Mb[(size_t)i * npad + col] = (T)lt[col][i];
    }
}

template <typename T>
__device__ __forceinline__ void leaf_store_w_rows(T* __restrict__ Wb, int npad, double (*w)[LEAF_LDT], int a, int lane) {
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int i = a * 16 + m;
        Wb[(size_t)i * npad + lane] = (T)(lane <= i ? w[i][lane] : 0.0);
    }
}

template <typename T, bool FROM_LDS>
__device__ __forceinline__ void leaf_factor_invert(T* __restrict__ Mb, T* __restrict__ Wb, int npad, double (*lt)[LEAF_LDT],
                                                   double (*w)[LEAF_LDT], double* scratch, double* dinv, double* pivs,
                                                   int* bad, int jb) {
    const int tid = body_tid(), lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lq = lane >> 4;
    d4 acc[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            // FROM_LDS: the caller left the block in the w area (w itself is first written after the first barrier below)
            acc[rb][e] = rb < wv ? 0.0 : FROM_LDS ? w[rb * 16 + lq + 4 * e][wv * 16 + li]
                                                  : (double)Mb[(size_t)(rb * 16 + lq + 4 * e) * npad + wv * 16 + li];
    double (*S)[17] = (double (*)[17])scratch;
    int first_bad = 0;
#pragma unroll 1
    for (int kb = 0; kb < 4; ++kb) {
        if (wv == kb) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (rb >= kb) S[rb * 16 + lq + 4 * e][li] = acc[rb][e];
            const int nlow = 3 - kb;                  // 16-row blocks below the diagonal block of this panel
            const int base = kb * 16;
            double rD[16], rL[16];
            const int lrow = lq < nlow ? base + 16 * (1 + lq) + li : base + li;      // (unconditional read, then select)
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                rD[c] = S[base + li][c];
                const double below = S[lrow][c];
                rL[c] = lq < nlow ? below : 0.0;
            }
            double dmine = 1.0;                       // the pivot of row li of the diagonal block
            PivotSteps<0>::run(rD, rL, dmine, li);
            const double rsl = fast_rsqrt(dmine);     // off the chain
            ScaleCols<0>::run(rD, rL, rsl);
            if (lq == 0) { dinv[base + li] = rsl; pivs[base + li] = dmine; }
            const unsigned long long bm = __ballot(!(dmine > 0.0)) & 0xffffull;
            if (bm) first_bad = jb * TS + base + __ffsll((long long)bm);
            // lt[col][row], all 64 rows of the panel's 16 columns in ONE pass of 16 stores: the four lane rows are exactly the
            // nlow blocks below the diagonal block (lane rows 0 .. nlow-1), the diagonal block itself (lane row nlow: rD is
            // the same in every lane row; zero above the diagonal) and the kb zero blocks above it (the remaining lane rows)
            const int row = lq < nlow ? base + 16 * (1 + lq) + li : lq == nlow ? base + li : 16 * (lq - nlow - 1) + li;
#pragma unroll
            for (int m = 0; m < 16; ++m)
                lt[base + m][row] = lq < nlow ? rL[m] : (lq == nlow && li >= m) ? rD[m] : 0.0;
            if (lane == 0) bad[kb] = first_bad;
        } else if (wv == kb - 1) {
            // row kb-1 of the inverse (panel kb-1 and everything it needs became visible at the last barrier)
            const int a = kb - 1;
            leaf_inverse_diag(lt, w, dinv, a, lane);
            for (int b = 0; b < a; ++b) {
                const d4 tacc = leaf_inverse_t(lt, w, a, b, lane);
                leaf_inverse_w(w, tacc, a, b, lane);
            }
        } else if (kb == 0) {
            // the 128x128 tile kernels read whole diagonal 128-blocks of W: keep the quadrant above this block zero
            if ((jb & 1) == 0)
                for (int i = wv - 1; i < TS; i += 3) Wb[(size_t)i * npad + TS + lane] = (T)0;
        } else if (wv == ((kb + 1) & 3)) {
            leaf_store_l_panel<T>(Mb, npad, lt, kb - 1, lane);
        } else if (kb >= 2 && wv == ((kb + 2) & 3)) {
            leaf_store_w_rows<T>(Wb, npad, w, kb - 2, lane);
        }
        __syncthreads();
        if (wv > kb) {
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const double bv = lt[kb * 16 + 4 * st + lq][wv * 16 + li];
#pragma unroll
                for (int rb = 1; rb < 4; ++rb)
                    if (rb >= wv)
                        acc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(-lt[kb * 16 + 4 * st + lq][rb * 16 + li], bv, acc[rb],
                                                                       0, 0, 0);
            }
        }
    }
    // row 3 of the inverse: W_33 on wave 3, T_3b = sum_m L_3m W_mb on wave b (b = 0, 1, 2), then W_3b = -W_33 T_3b
    d4 tacc = {0.0, 0.0, 0.0, 0.0};
    if (wv == 3) leaf_inverse_diag(lt, w, dinv, 3, lane);
    else tacc = leaf_inverse_t(lt, w, 3, wv, lane);
    __syncthreads();
    if (wv < 3) leaf_inverse_w(w, tacc, 3, wv, lane);
    else leaf_store_l_panel<T>(Mb, npad, lt, 3, lane);
    __syncthreads();
    if (wv == 1) leaf_store_w_rows<T>(Wb, npad, w, 2, lane);
    else if (wv == 2) leaf_store_w_rows<T>(Wb, npad, w, 3, lane);
}

template <typename T, bool FROM_LDS = false>
__device__ __forceinline__ void leaf_body(unsigned char* lds, int k, T* __restrict__ M, T* __restrict__ W, size_t mat,
                                          int npad, int jb, double* __restrict__ logdet, int* __restrict__ info) {
    double (*lt)[LEAF_LDT] = (double (*)[LEAF_LDT])lds;                   // lt[col][row] = L[row][col]
    double (*w)[LEAF_LDT] = (double (*)[LEAF_LDT])((double*)lds + TS * LEAF_LDT);     // w[row][col] = (L^-1)[row][col]
    double* scratch = (double*)lds + 2 * TS * LEAF_LDT;
    double* dinv = scratch + LEAF_SCR;
    double* pivs = dinv + TS;
    int* bad = (int*)(pivs + TS);
    const int tid = body_tid();
    T* Mb = M + (size_t)k * mat + (size_t)jb * TS * npad + (size_t)jb * TS;
    T* Wb = W + (size_t)k * mat + (size_t)jb * TS * npad + (size_t)jb * TS;
    // the running log-determinant and status of the component are fetched now, so that the end is a store, not a round trip
    double ld_prev = 0.0;
    int info_prev = 0;
    if (tid == 0) { ld_prev = logdet[k]; info_prev = info[k]; }
    leaf_factor_invert<T, FROM_LDS>(Mb, Wb, npad, lt, w, scratch, dinv, pivs, bad, jb);
    if (tid < TS) {   // wave 0 (the other waves are storing the last rows): 1/2 sum log(pivot)
        double lg = 0.5 * log(pivs[tid]);
        for (int off = 32; off > 0; off >>= 1) lg += __shfl_xor(lg, off);
        if (tid == 0) {
            logdet[k] = ld_prev + lg;
            const int fb = bad[0] ? bad[0] : bad[1] ? bad[1] : bad[2] ? bad[2] : bad[3];
            if (fb && info_prev == 0) info[k] = fb;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void leaf_kernel(T* __restrict__ M, T* __restrict__ W, size_t mat, int npad, int jb,
                                                   double* __restrict__ logdet, int* __restrict__ info) {
    __shared__ __align__(16) unsigned char lds[LEAF_LDS_BYTES];
    leaf_body<T>(lds, blockIdx.x, M, W, mat, npad, jb, logdet, info);
}

// ---------------------------------------------------------------------------------------------------
// Tile GEMM on MFMA:  C_tile (op)= alpha * sum_kt  Aop(kt) * Bop(kt)^T,   64x64 output per workgroup,
// 4 waves each owning a 32x32 quadrant (2x2 MFMA 16x16x4 accumulators).  Operand tiles are 64 x 64
// sub-blocks of M / W / V, read in either orientation:
//   MK : element (m, k) at P[m * ld + k]      KM : element (m, k) at P[k * ld + m]
// and staged in LDS as [k][m] (KT = 16 k rows per stage, double buffered through registers).
// ---------------------------------------------------------------------------------------------------
enum GemmOp { OP_SYRK = 1, OP_TRTRI_T = 2, OP_TRTRI_W = 3, OP_LAUUM = 4, OP_PRED_U = 5, OP_PRED_COV = 6, OP_PRED_V = 7, OP_VR = 8,
              OP_VG_P = 9, OP_VG_G = 10, OP_HESS_G = 11, OP_COND_CROSS = 12, OP_COND_U = 13 };
enum Lay { MK = 0, KM = 1 };

struct GemmArgs {
    const void* A; const void* B; void* C;     // component-0 bases
    size_t sA, sB, sC;                          // per-component strides (elements)
    int ldA, ldB, ldC;
    int nb;                                     // number of 64-blocks
    int p0, p1, p2, p3;                         // op specific
    int q;                                      // components in this launch
    int t0;                                     // first tile of this launch (OP_SYRK)
    int skipq;                                  // OP_SYRK on 128-tiles: tile 0 leaves its top-left 64x64 quadrant alone
                                                // (the diagonal block there is factored by the same launch, wide_leaf_kernel)
    const void* bvec = nullptr;                 // OP_LAUUM on 128-tiles: b (npad per component) and the partial buffer of
    double* part = nullptr;                     // z = A^-1 b, [component][tile][2][128]; null = no fused product
    unsigned long long* clk = nullptr;          // OP_LAUUM: the first block (the longest K loop of the launch) leaves its duration
                                                // in shader-clock cycles and in 10 ns ticks here: the clock the chip held (lcgp_lauum_clock)
    const double* theta = nullptr;              // OP_PRED_COV: theta rows, p1 doubles apart; D_k is element p2 of row k
                                                // (OP_VR: rows tw apart; OP_COND_CROSS: rows p2 apart, D_k element p3)
    // OP_VR (the variance-reduction epilogue; see vr_epilogue): standardised inputs of the A rows (reference set) and of the
    // B rows (candidates), d per row; the weights of the reference rows; the candidates' gvar (ldg per component); the covariance
    // kernel, theta row width, replicates r and the row length of the partial sums (p0 = k tiles, p1 = candidate tiles,
    // p2 = n_ref, p3 = n_cand)
    const void* xa = nullptr;
    const void* xb = nullptr;
    const double* wref = nullptr;
    const double* gvc = nullptr;
    int ldg = 0, d = 0, kern = 0, tw = 0, nrep = 1, ldp = 0;
};

// one K-stage (KT = 16 k values) of a TM-row operand tile: global -> registers -> LDS [k][m], ld = TM + 16;
// NT threads move TM * KT elements, EPT = TM * KT / NT consecutive ones each
// LDS image of a stage: [k][m] with row length LD = TM + 16 (= 16 mod 32 doubles: the two k rows a 32-lane ds_read_b64
// group touches lie in disjoint bank halves) and the column index XOR-ed with (k & 12).  The XOR is what makes the
// TRANSPOSING store of a k-contiguous operand (MK: a lane holds 4 consecutive k of one row m) conflict-free: a
// ds_write_b64 is served in groups of 16 contiguous lanes over 32 banks (MI355X_MICROARCH.md, LDS), and those 16 lanes
// are 4 rows m x 4 k-quads -- without the XOR all four quads of a row hit one bank pair (4-way conflict on every
// store of every stage; same-box A/B: 11.20 -> 10.95 ms per evaluation).  Within one k row the XOR only permutes each
// aligned group of 16 columns, so the fragment reads (16 consecutive columns of one row) stay conflict-free, and for
// the m-contiguous operand layout (KM: 16-byte pieces per lane) it moves whole aligned pieces, so the 16-byte stores stay.
// In float the banks are per 4 bytes and a ds_write_b32 group is 32 lanes = 8 rows x 4 k-quads: the XOR constants are
// 0, 8, 16, 24 there (they exchange whole 16-column groups inside a wave's 32-aligned sub-tile: the read side applies
// the XOR to the column index relative to the sub-tile origin, which is a multiple of 32).
template <typename T>
__device__ __forceinline__ constexpr int lds_swz(int k) { return (k & 12) * (int)(8 / sizeof(T)); }   // float: 0, 8, 16, 24
static_assert(KT == 16, "lds_swz assumes 16 k rows per stage");
// Swizzled column of a fragment read: 16-group `g16` (a multiple of 16, compile-time after unrolling) + lane column l15 of
// k step kk.  The XOR splits into a part that exchanges whole 16-groups (compile-time: folds into the instruction's
// offset) and a part inside the group (lane-dependent: one register per distinct constant).
template <typename T>
__device__ __forceinline__ int swz_col(int g16, int l15, int kk) {
    return (g16 ^ (lds_swz<T>(4 * kk) & ~15)) + (l15 ^ (lds_swz<T>(4 * kk) & 15));
}

template <typename T, int L, int TM, int NT>
__device__ __forceinline__ void load_stage(const T* __restrict__ P, int ld, int ks, T (&reg)[TM * KT / NT], int tid) {
    constexpr int EPT = TM * KT / NT;
    if (L == MK) {
        constexpr int TPR = KT / EPT;                       // threads per operand row (a row holds 16 k values)
        const int m = tid / TPR, kk = (tid % TPR) * EPT;
        const T* src = P + (size_t)m * ld + ks + kk;
#pragma unroll
        for (int e = 0; e < EPT; ++e) reg[e] = src[e];
    } else {
        // a lane holds EPT / PE pieces of 16 bytes; piece p of the lanes of one k row is one contiguous run (so that the
        // 8-lane groups of the ds_write_b128 that stores it cover 128 contiguous bytes = all 32 banks once; with four
        // consecutive doubles per lane, lanes l and l + 4 of a group shared their banks: 2-way conflict on every store)
        constexpr int TPK = TM / EPT;                       // threads per k row
        constexpr int PE = 16 / (int)sizeof(T), NP = EPT / PE;
        const int kq = tid / TPK, j = tid % TPK;
        const T* src = P + (size_t)(ks + kq) * ld + j * PE;
#pragma unroll
        for (int pc = 0; pc < NP; ++pc)
#pragma unroll
            for (int e = 0; e < PE; ++e) reg[pc * PE + e] = src[pc * (TM / NP) + e];
    }
}

template <typename T, int L, int TM, int NT>
__device__ __forceinline__ void store_stage(T* __restrict__ S, const T (&reg)[TM * KT / NT], int tid) {
    constexpr int EPT = TM * KT / NT;
    constexpr int LD = TM + 16;
    if (L == MK) {
        constexpr int TPR = KT / EPT;
        const int m = tid / TPR, kk = (tid % TPR) * EPT;
#pragma unroll
        for (int e = 0; e < EPT; ++e) S[(kk + e) * LD + (m ^ lds_swz<T>(kk + e))] = reg[e];
    } else {
        constexpr int TPK = TM / EPT;
        constexpr int PE = 16 / (int)sizeof(T), NP = EPT / PE;
        const int kq = tid / TPK, j = tid % TPK;
#pragma unroll
        for (int pc = 0; pc < NP; ++pc)
#pragma unroll
            for (int e = 0; e < PE; ++e) S[kq * LD + ((j * PE + pc * (TM / NP)) ^ lds_swz<T>(kq)) + e] = reg[pc * PE + e];
    }
}

// ---- hand-counted operand prefetch (the triangular products of the inverse) ----
// hipcc's wait-count pass puts `s_waitcnt vmcnt(3..0)` in front of the first LDS store of every double stage of the register
// prefetch loop below, although the set being stored is the OLDER of two outstanding ones (it needs vmcnt(4..7)): the stage
// fetched one compute stage ago is waited for as well and the second stage of prefetch covers no latency (the pass is
// conservative at the loop header whether or not the loads sit under a condition; the same loop with unconditional loads
// compiles to the same waits).  So the loads of that loop are issued through inline asm, which the pass does not track, and
// the waits are written out: vector-memory operations retire in order, so with PF sets of NL loads outstanding the oldest
// set is complete at vmcnt((PF - 1) NL).  The asm that waits takes the set's registers as read-write operands, so every
// use of them is ordered behind it.  Compiler-generated waits stay correct beside this (they can only wait for more).
template <typename T> struct Piece;
template <> struct Piece<double> { typedef double v __attribute__((ext_vector_type(2))); };
template <> struct Piece<float> { typedef float v __attribute__((ext_vector_type(4))); };

// one 16-byte piece: address = wave-uniform base (SGPR pair) + per-lane byte offset (one VGPR, loop-invariant) + immediate.
// The scalar base keeps the whole address arithmetic of a stage on the scalar unit: the fp64 128-tile kernels sit at the
// 128-register limit of four waves per SIMD, and 64-bit per-lane pointers spilled there (a spill reload inside the K loop
// is a scratch load, i.e. a vmcnt(0) wait for every prefetched stage).
template <int IMM, typename P>
__device__ __forceinline__ void gload_piece(P& dst, unsigned voff, const void* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(IMM) : "memory");
}

template <int N, typename P>
__device__ __forceinline__ void vm_wait_set(P (&a)[1], P (&b)[1]) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a[0]), "+v"(b[0]) : "n"(N) : "memory");
}
template <int N, typename P>
__device__ __forceinline__ void vm_wait_set(P (&a)[4], P (&b)[4]) {
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
                 : "n"(N) : "memory");
}
template <int N, typename P>
__device__ __forceinline__ void vm_wait_set(P (&a)[2], P (&b)[2]) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]) : "n"(N) : "memory");
}

// the same stage image as load_stage / store_stage, the registers as 16-byte pieces (NPC = EPT sizeof(T) / 16 per lane)
// byte offset of this lane's first piece within a stage of an operand tile
template <typename T, int L, int TM, int NT>
__device__ __forceinline__ unsigned stage_lane_offset(int ld, int tid) {
    constexpr int EPT = TM * KT / NT;
    constexpr int PE = 16 / (int)sizeof(T);
    if (L == MK) {
        constexpr int TPR = KT / EPT;
        const int m = tid / TPR, kk = (tid % TPR) * EPT;
        return (unsigned)((m * ld + kk) * (int)sizeof(T));
    } else {
        constexpr int TPK = TM / EPT;
        const int kq = tid / TPK, j = tid % TPK;
        return (unsigned)((kq * ld + j * PE) * (int)sizeof(T));
    }
}

// load_stage with the address split into a wave-uniform base (scalar registers) and this lane's offset within a stage
// (stage_lane_offset, bytes; loop-invariant): the compiler then uses the scalar-base form of global_load and no per-lane
// 64-bit pointer lives across the K loop
template <typename T, int L, int TM, int NT>
__device__ __forceinline__ void load_stage_u(const T* __restrict__ P /*wave-uniform*/, int ld, int ks, T (&reg)[TM * KT / NT],
                                             unsigned voff) {
    constexpr int EPT = TM * KT / NT;
    const T* src = (const T*)((const char*)(L == MK ? P + ks : P + (size_t)ks * ld) + voff);
    if (L == MK) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) reg[e] = src[e];
    } else {
        constexpr int PE = 16 / (int)sizeof(T), NP = EPT / PE;
#pragma unroll
        for (int pc = 0; pc < NP; ++pc)
#pragma unroll
            for (int e = 0; e < PE; ++e) reg[pc * PE + e] = src[pc * (TM / NP) + e];
    }
}

template <typename T, int L, int TM, int NT, int PC = 0>
__device__ __forceinline__ void load_stage_p(const T* __restrict__ P /*wave-uniform*/, int ld, int ks,
                                             typename Piece<T>::v (&reg)[TM * KT / NT * (int)sizeof(T) / 16], unsigned voff) {
    constexpr int EPT = TM * KT / NT;
    constexpr int PE = 16 / (int)sizeof(T), NP = EPT / PE;
    const T* base = L == MK ? P + ks : P + (size_t)ks * ld;
    constexpr int STEP = (L == MK ? PE : TM / NP) * (int)sizeof(T);      // bytes between the pieces of a lane
    if constexpr (PC < NP) {
        gload_piece<PC * STEP>(reg[PC], voff, base);
        load_stage_p<T, L, TM, NT, PC + 1>(P, ld, ks, reg, voff);
    }
}

template <typename T, int L, int TM, int NT>
__device__ __forceinline__ void store_stage_p(T* __restrict__ S, const typename Piece<T>::v (&reg)[TM * KT / NT * (int)sizeof(T) / 16],
                                              int tid) {
    constexpr int EPT = TM * KT / NT;
    constexpr int LD = TM + 16;
    constexpr int PE = 16 / (int)sizeof(T), NP = EPT / PE;
    if (L == MK) {
        constexpr int TPR = KT / EPT;
        const int m = tid / TPR, kk = (tid % TPR) * EPT;
#pragma unroll
        for (int e = 0; e < EPT; ++e) S[(kk + e) * LD + (m ^ lds_swz<T>(kk + e))] = reg[e / PE][e % PE];
    } else {
        constexpr int TPK = TM / EPT;
        const int kq = tid / TPK, j = tid % TPK;
#pragma unroll
        for (int pc = 0; pc < NP; ++pc)
            *(typename Piece<T>::v*)&S[kq * LD + ((j * PE + pc * (TM / NP)) ^ lds_swz<T>(kq))] = reg[pc];
    }
}

// ---- row image of a k-contiguous fp64 operand (gemm_body only) ----
// A k-contiguous operand (MK: a lane holds 4 consecutive k of one row m) went into the [k][m] image through a TRANSPOSING
// store: four ds_write_b64 per lane, operand and stage, behind the XOR that makes them conflict-free.  Kept as it lies in
// memory instead -- S[m * LDK + k], LDK = KT + 2 doubles -- a lane stores its 32 bytes as two 16-byte pieces (half the LDS
// store instructions, whose issue + wait + barrier in front of every stage cost the rank-256 update 18 % of its time:
// profiles/r06_syrk_destructive.txt) and the TRANSPOSITION moves to the fragment read, where it is free: lane (i, kq) of an
// MFMA operand reads S[(m0 + i) LDK + k0 + kq], and with 36 dwords per row the 16 rows of a 32-lane ds_read_b64 group start
// on 16 different multiples of 4 banks (36 i mod 64), two banks each, the second k of the group two banks further: all 64
// banks once.  One address register per operand (the swizzled [k][m] image needs one per k step).
constexpr int LDK = KT + 2;
template <int TM, int NT>
__device__ __forceinline__ void store_stage_rows(double* __restrict__ S, const double (&reg)[TM * KT / NT], int tid) {
    constexpr int EPT = TM * KT / NT, TPR = KT / EPT;
    typedef double d2 __attribute__((ext_vector_type(2)));
    const int m = tid / TPR, kk = (tid % TPR) * EPT;
#pragma unroll
    for (int pc = 0; pc < EPT / 2; ++pc) *(d2*)&S[m * LDK + kk + 2 * pc] = d2{reg[2 * pc], reg[2 * pc + 1]};
}
template <int TM, int NT>
__device__ __forceinline__ void store_stage_rows_p(double* __restrict__ S, const Piece<double>::v (&reg)[TM * KT / NT / 2], int tid) {
    constexpr int EPT = TM * KT / NT, TPR = KT / EPT;
    const int m = tid / TPR, kk = (tid % TPR) * EPT;
#pragma unroll
    for (int pc = 0; pc < EPT / 2; ++pc) *(Piece<double>::v*)&S[m * LDK + kk + 2 * pc] = reg[pc];
}

// Workgroups are dealt round-robin over the 8 XCDs (each with its own L2).  Remap the linear tile id so that
// every XCD works on one contiguous run of tiles (neighbouring tiles share operand panels): bijective for any
// grid size (speed only, never correctness).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7, i = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ---- OP_VR epilogue: integrated variance reduction (lcgp_hip.h: lcgp_variance_reduction) ----
// For reference tile rt, candidate tile ct and component k the accumulators hold acc[t, c] = U_k(t) . U_k(c); then
//   sigma(t, c)    = C_k(t, c) - D_k acc[t, c]          C_k without nugget (reference points are new inputs)
//   part[k, rt, c] = (sum_t w_t sigma^2) / den_c,       den_c = max(gvar_c, 0) + 1 / (D_k r)
// C_k is recomputed in double from the standardised inputs of the tile's rows and columns, staged in LDS divided by ell
// (the stage buffers are free behind the k loop) VR_DC dimensions at a time, as cross_kernel forms it.  Row sums in a fixed
// order: per lane over its registers, then the four lanes 16 apart (they hold the same column: row = (lane >> 4) + 4 reg in
// fp64, 4 (lane >> 4) + reg in fp32), then the lower pair of waves hands its sums to the upper pair through LDS.
// Reference rows beyond n_ref carry weight 0; candidate columns beyond n_cand are not written.
constexpr int VR_DC = 16;
template <typename T, int KERN, int TM, int MIM, int MIN, typename Acc>
__device__ __forceinline__ void vr_epilogue(const GemmArgs& g, const Acc (&acc)[MIM][MIN], int k, int rt, int ct, int tid, int wm0,
                                            int wn0, unsigned char* lds) {
    static_assert(TM == 64 && MIM == 2 && MIN == 2, "the OP_VR epilogue is written for the 64x64 tile on four waves");
    constexpr int XL = VR_DC + 1;                   // odd row length: the 16 rows a lane group reads hit distinct banks
    double* xa = (double*)lds;                      // [TM][XL] reference rows / ell
    double* xb = xa + TM * XL;                      // [TM][XL] candidate rows / ell
    double* wr = xb + TM * XL;                      // [TM] weights of the reference rows
    double* red = wr + TM;                          // [TM] column sums of the waves that own rows 32 .. 63
    static_assert((2 * TM * XL + 2 * TM) * sizeof(double) <= 4 * KT * (TM + 16) * sizeof(T), "fits the stage buffers");
    const int lane = tid & 63, l15 = lane & 15, wave = tid >> 6;
    const int d = g.d;
    const double* th = g.theta + (size_t)k * g.tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double coff = scale * (1.0 - nug / (1.0 + nug));
    const T* xra = (const T*)g.xa;
    const T* xrb = (const T*)g.xb;
    const int t0 = rt * TM, c0 = ct * TM;
    __syncthreads();                                // every wave is done with the stage buffers
    if (tid < TM) wr[tid] = t0 + tid < g.p2 ? g.wref[t0 + tid] : 0.0;
    double s[MIN];
#pragma unroll
    for (int ni = 0; ni < MIN; ++ni) s[ni] = 0.0;
    const int nch = (d + VR_DC - 1) / VR_DC;
    // one 16 x 16 accumulator block at a time (four elements per lane): the kernel values of a block are accumulated over all
    // dimension chunks before the next block starts, so only its four (poly, sum) pairs live beside the accumulators
#pragma unroll
    for (int mi = 0; mi < MIM; ++mi)
#pragma unroll
        for (int ni = 0; ni < MIN; ++ni) {
            double pl[4], ss[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { pl[e] = 1.0; ss[e] = 0.0; }
            // (loops over dimensions and staged elements kept rolled: unrolled, the compiler hoists their LDS reads and global
            // loads ahead of the arithmetic and runs out of the 128 registers four waves per SIMD leave)
#pragma unroll 1
            for (int ch = 0; ch < nch; ++ch) {
                const int d0 = ch * VR_DC, dc = d - d0 < VR_DC ? d - d0 : VR_DC;
                if (nch > 1 || (mi == 0 && ni == 0)) {      // (one chunk: staged once for all blocks)
                    if (ch > 0 || mi > 0 || ni > 0) __syncthreads();
#pragma unroll 1
                    for (int e = tid; e < TM * VR_DC; e += 256) {
                        const int i = e / VR_DC, j = e - i * VR_DC;
                        const int ta = t0 + i, cb = c0 + i;
                        xa[i * XL + j] = (j < dc && ta < g.p2) ? (double)xra[(size_t)ta * d + d0 + j] / th[d0 + j] : 0.0;
                        xb[i * XL + j] = (j < dc && cb < g.p3) ? (double)xrb[(size_t)cb * d + d0 + j] / th[d0 + j] : 0.0;
                    }
                    __syncthreads();
                }
                const double* pa = xa + (wm0 + mi * 16) * XL;
                const double* pb = xb + (wn0 + ni * 16 + l15) * XL;
#pragma unroll 1
                for (int jj = 0; jj < dc; ++jj) {
                    const double yv = pb[jj];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double xv = pa[Mfma<T>::row(lane, e) * XL + jj];
                        if constexpr (KERN == 0) {
                            const double sd = fabs(xv - yv);
                            pl[e] = fma(pl[e], sd, pl[e]);
                            ss[e] -= sd;
                        } else if constexpr (KERN == 1) {
                            const double df = xv - yv;
                            ss[e] = fma(-0.5 * df, df, ss[e]);
                        } else {
                            static_assert(KERN == 2, "unknown covariance kernel id");
                            const double sd = fabs(xv - yv);
                            pl[e] = fma(pl[e], m52_fm1(sd), pl[e]);
                            ss[e] -= sd;
                        }
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double c = kern_c0<KERN>(pl[e], ss[e]);
                const double sg = fma(-D, (double)acc[mi][ni][e], coff * c);
                s[ni] = fma(wr[wm0 + mi * 16 + Mfma<T>::row(lane, e)] * sg, sg, s[ni]);
            }
        }
#pragma unroll
    for (int ni = 0; ni < MIN; ++ni) {
        s[ni] += __shfl_xor(s[ni], 16);
        s[ni] += __shfl_xor(s[ni], 32);
    }
    if (wave >= 2 && lane < 16) {
#pragma unroll
        for (int ni = 0; ni < MIN; ++ni) red[wn0 + ni * 16 + l15] = s[ni];
    }
    __syncthreads();
    if (wave < 2 && lane < 16) {
        const double rd = 1.0 / (D * (double)g.nrep);
        double* part = (double*)g.C + ((size_t)k * ((g.p2 + TM - 1) / TM) + rt) * g.ldp;
#pragma unroll
        for (int ni = 0; ni < MIN; ++ni) {
            const int cl = wn0 + ni * 16 + l15, c = c0 + cl;
            if (c < g.p3) part[c] = (s[ni] + red[cl]) / (fmax(g.gvc[(size_t)k * g.ldg + c], 0.0) + rd);
        }
    }
}

// TM x TM output tile per workgroup of NW waves arranged (NW/2) x 2:
//   TM = 64,  NW = 4: 32x32 per wave (2x2 MFMA accumulators), 4 workgroups per CU
//   TM = 128, NW = 8: 32x64 per wave (2x4 accumulators), 2 workgroups per CU = 4 waves per SIMD, half the
//                     operand traffic per flop of the 64-tile
// All tile coordinates (g.nb, g.p0..p3) are in units of TM.
template <typename T, int OP, int TM, int NW>
__device__ __forceinline__ void gemm_body(const GemmArgs& g, const int lin /*block index within this descriptor*/,
                                          unsigned char* lds) {
    constexpr int LA = (OP == OP_LAUUM) ? KM : MK;
    constexpr int LB = (OP == OP_TRTRI_T || OP == OP_TRTRI_W || OP == OP_LAUUM || OP == OP_PRED_V || OP == OP_VG_G || OP == OP_HESS_G ||
                        OP == OP_COND_U) ? KM : MK;
    constexpr int NT = NW * 64;
    constexpr int LD = TM + 16;     // = 16 (mod 32): the two k rows a 32-lane group reads hit disjoint banks
    constexpr int WTM = TM / (NW / 2), WTN = TM / 2;   // per-wave sub-tile
    constexpr int MIM = WTM / 16, MIN = WTN / 16;      // MFMA tiles per wave
    constexpr int EPT = TM * KT / NT;
    T* As = (T*)lds;                  // [2][KT * LD]
    T* Bs = As + 2 * KT * LD;         // [2][KT * LD]

    // (tile, component) with the component as the FAST index: tiles are enumerated heaviest first, so the heaviest
    // tiles of every component start at once instead of component by component
    int lin_ = lin;
    if constexpr (OP == OP_TRTRI_T || OP == OP_TRTRI_W || OP == OP_LAUUM) {
        // With few components a launch of the triangular products is one or two rounds of resident workgroups, so its
        // time is the k length a CU collects from the tiles it hosts together.  Workgroups go to the CUs round-robin
        // (workgroup b and b + 256 share a CU): every other group of 256 is enumerated backwards, which pairs the
        // heaviest tiles with the lightest ones (first round at n = 4096, one component: 80 k tiles on the fullest CU
        // in plain heaviest-first order, 66 on every CU this way; same-box A/B: 2.80 -> 2.73 ms at one component, 3.93 ->
        // 3.91 at two, nothing at four).  With many components the launches have many rounds, and with 8 the component
        // index doubles as the XCD index (L2 locality), which the reversal would break.
        if (g.q < 4 && !g.skipq && ((lin >> 8) & 1)) {      // (skipq: the body runs as a filler job, gridDim is not its own)
            const int base = lin & ~255, nblk = (int)gridDim.x;
            const int top = base + 255 < nblk ? base + 255 : nblk - 1;      // last index of this (possibly short) group
            lin_ = top - (lin - base);
        }
    }
    const int k = lin_ % g.q;
    const int bid = lin_ / g.q;
    const T* Ab = (const T*)g.A + (size_t)k * g.sA;
    const T* Bb = (const T*)g.B + (size_t)k * g.sB;
    T* Cb = (T*)g.C + (size_t)k * g.sC;

    // ---- per-op tile decode: A0/B0 = first operand tiles, dA/dB = pointer step per kt, nkt, C tile ----
    const T* A0; const T* B0; T* Ct;
    ptrdiff_t dA, dB;           // signed: some ops walk their k tiles downwards (see below)
    int nkt;
    double alpha = 1.0;
    bool accumulate = false;
    bool tri_b = false;         // OP_LAUUM: the B operand of the last k tile is triangular too (diagonal tile)
    if constexpr (OP == OP_SYRK) {
        // M[r, c] -= sum_{kt in [p0, p1)} M[r, kt] M[c, kt]^T over the tiles c in [p2, p3), r in [c, nb)
        // (p3 == nb: the whole trailing triangle; p3 < nb: the rest of the current panel)
        // Band-major: the rows p2 + i in bands of SB; inside a band column by column.  The workgroups resident on an XCD at
        // one time (with eight components the component IS the XCD) then cover SB row tiles x a dozen column tiles instead
        // of ~100 row tiles of one column: their operand panels (SB + a dozen of them) stay in the XCD's 4 MB L2, where a
        // column-major order re-fetched a row panel per tile (profiles/r06_hbm_traffic_per_kernel.txt: 7.2 GB per
        // evaluation through the fabric for 1.07 GB of matrix).  Same tiles, same arithmetic per tile.
        constexpr int SB = 8;
        int t = bid + g.t0, r;
        int i0 = 0;                                   // first row of the band, relative to p2
        for (;;) {
            // tiles of the band [i0, i0 + SB): row p2 + i holds the columns p2 .. min(p2 + i, p3 - 1)
            const int rows = g.nb - g.p2 - i0 < SB ? g.nb - g.p2 - i0 : SB;
            int cnt = 0;
            for (int i = i0; i < i0 + rows; ++i) cnt += (i < g.p3 - g.p2 ? i : g.p3 - g.p2 - 1) + 1;
            if (t < cnt) break;
            t -= cnt;
            i0 += SB;
        }
        const int rows = g.nb - g.p2 - i0 < SB ? g.nb - g.p2 - i0 : SB;
        // column j (relative) of the band holds the rows max(j, i0) .. i0 + rows - 1
        int j = 0;
        for (;;) {
            const int lo = j > i0 ? j : i0;
            const int cnt = i0 + rows - lo;
            if (t < cnt) { r = g.p2 + lo + t; break; }
            t -= cnt;
            ++j;
        }
        const int c = g.p2 + j;
        A0 = Ab + (size_t)r * TM * g.ldA + (size_t)g.p0 * TM; dA = TM;
        B0 = Bb + (size_t)c * TM * g.ldB + (size_t)g.p0 * TM; dB = TM;
        nkt = g.p1 - g.p0;
        Ct = Cb + (size_t)r * TM * g.ldC + (size_t)c * TM;
        alpha = -1.0; accumulate = true;
    } else if constexpr (OP == OP_TRTRI_T || OP == OP_TRTRI_W) {
        // level with block size mb = p0: pair pr covers block rows [2 pr mb, 2 pr mb + 2 mb).
        // Tiles are enumerated longest-k-loop first (T: cl ascending, W21: rl descending; the pair index is the
        // fastest one) so that the long tiles start early and the short ones fill the tail.
        const int mb = g.p0;
        const int npair = g.p1;
        const int pr = g.p2 + bid % npair, rem = bid / npair;      // p2 = first pair (0 for a whole level)
        int rl, cl;
        if constexpr (OP == OP_TRTRI_T) { cl = rem / mb; rl = rem - cl * mb; }
        else { rl = mb - 1 - rem / mb; cl = rem % mb; }
        const int C0 = 2 * pr * mb, R0 = C0 + mb;
        if (R0 + rl >= g.nb) return;
        if constexpr (OP == OP_TRTRI_T) {
            // T[rl, cl] = sum_{kt = cl}^{mb-1} L21[rl, kt] W11[kt, cl]          (A from M, B from W, C into V)
            // walked from kt = mb-1 DOWN to cl: all tiles of the launch start on the same block row of W11 and
            // the same block column of L21 and stay in step, so the per-XCD L2 serves the re-reads
            A0 = Ab + (size_t)(R0 + rl) * TM * g.ldA + (size_t)(C0 + mb - 1) * TM; dA = -(ptrdiff_t)TM;
            B0 = Bb + (size_t)(C0 + mb - 1) * TM * g.ldB + (size_t)(C0 + cl) * TM; dB = -(ptrdiff_t)TM * g.ldB;
            nkt = mb - cl;
        } else {
            // W21[rl, cl] = - sum_{kt = 0}^{rl} W22[rl, kt] T[kt, cl]            (A from W, B from V, C into W)
            A0 = Ab + (size_t)(R0 + rl) * TM * g.ldA + (size_t)R0 * TM; dA = TM;
            B0 = Bb + (size_t)R0 * TM * g.ldB + (size_t)(C0 + cl) * TM; dB = (ptrdiff_t)TM * g.ldB;
            nkt = rl + 1;
            alpha = -1.0;
        }
        Ct = Cb + (size_t)(R0 + rl) * TM * g.ldC + (size_t)(C0 + cl) * TM;
    } else if constexpr (OP == OP_LAUUM) {
        // V[r, c] = sum_{kt = r}^{nb-1} W[kt, r]^T W[kt, c]
        int r, c;
        tri_decode(bid, r, c);   // ascending r = longest k loops first
        // k tiles walked from nb-1 DOWN to r: every tile starts on the last block row of W and they stay in step
        A0 = Ab + (size_t)(g.nb - 1) * TM * g.ldA + (size_t)r * TM; dA = -(ptrdiff_t)TM * g.ldA;
        B0 = Bb + (size_t)(g.nb - 1) * TM * g.ldB + (size_t)c * TM; dB = -(ptrdiff_t)TM * g.ldB;
        nkt = g.nb - r;
        tri_b = r == c;
        Ct = Cb + (size_t)r * TM * g.ldC + (size_t)c * TM;
    } else if constexpr (OP == OP_PRED_COV) {
        // C[r, c] -= D_k sum_{kt < p0} U[r, kt] U[c, kt]^T over the lower tiles c <= r   (U = n0pad x npad, p0 = npad / TM)
        int r, c;
        tri_decode(bid, r, c);
        A0 = Ab + (size_t)r * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)c * TM * g.ldB; dB = TM;
        nkt = g.p0;
        Ct = Cb + (size_t)r * TM * g.ldC + (size_t)c * TM;
        accumulate = true;          // (alpha = -D_k is read behind the k loop: nothing more lives across it than in OP_PRED_U)
    } else if constexpr (OP == OP_VR) {
        // acc = sum_{kt < p0} U_ref[rt, kt] U_cand[ct, kt]^T over all (reference tile rt, candidate tile ct); C is the partial
        // buffer, written by the epilogue
        const int ct = bid % g.p1, rt = bid / g.p1;
        A0 = Ab + (size_t)rt * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)ct * TM * g.ldB; dB = TM;
        nkt = g.p0;
        Ct = Cb;
    } else if constexpr (OP == OP_VG_P) {
        // P[c, t] = sum_{kt < p0} U_cand[ct, kt] U_ref[rt, kt]^T over all (candidate tile ct, reference tile rt), p1 reference
        // tiles per candidate tile: the product OP_VR keeps in registers, stored (lcgp_variance_reduction_grad)
        const int rt = bid % g.p1, ct = bid / g.p1;
        A0 = Ab + (size_t)ct * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)rt * TM * g.ldB; dB = TM;
        nkt = g.p0;
        Ct = Cb + (size_t)ct * TM * g.ldC + (size_t)rt * TM;
    } else if constexpr (OP == OP_COND_CROSS) {
        // C[r, c] -= D_k sum_{kt < p0} U_0[r, kt] U_n[c, kt]^T over ALL (row tile r of the new inputs, column tile c of the
        // conditioning inputs), p1 column tiles per row tile: the rectangular two-set sibling of OP_PRED_COV
        // (lcgp_condition_predict; C holds the kernel values C^x(x0, xn) on entry)
        const int c = bid % g.p1, r = bid / g.p1;
        A0 = Ab + (size_t)r * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)c * TM * g.ldB; dB = TM;
        nkt = g.p0;
        Ct = Cb + (size_t)r * TM * g.ldC + (size_t)c * TM;
        accumulate = true;          // (alpha = -D_k is read behind the k loop, as in OP_PRED_COV)
    } else if constexpr (OP == OP_VG_G || OP == OP_HESS_G) {
        // G[m, c] = sum_{kt < p1} S[m, kt] U_ref[kt, c]      (S = n_candpad x n_refpad, U_ref = n_refpad x npad: no triangle)
        // OP_HESS_G: the same dense product with dense square operands, G_i = A^-1 d_iA and Q = Y A^-1 of lcgp_nll_hess (A^-1
        // mirrored to a full matrix, d_iA materialised: neither operand has a triangle to skip)
        const int c = bid / g.p0, m = bid % g.p0;                  // p0 = row tiles of S
        A0 = Ab + (size_t)m * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)c * TM; dB = (ptrdiff_t)TM * g.ldB;
        nkt = g.p1;
        Ct = Cb + (size_t)m * TM * g.ldC + (size_t)c * TM;
    } else if constexpr (OP == OP_COND_U) {
        // U'[m, c] = U_0[m, c] - sum_{kt < p1} R[m, kt] U_n[kt, c]      (R = n0pad x mpad, U_n = mpad x npad, C = U_0 in place: the
        // rectangular product of OP_VG_G with K = mpad and the accumulating epilogue of OP_COND_CROSS, alpha = -1;
        // lcgp_condition_predict_grad).  Ascending k on either tile size.
        const int c = bid / g.p0, m = bid % g.p0;                  // p0 = row tiles of R
        A0 = Ab + (size_t)m * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)c * TM; dB = (ptrdiff_t)TM * g.ldB;
        nkt = g.p1;
        Ct = Cb + (size_t)m * TM * g.ldC + (size_t)c * TM;
        alpha = -1.0; accumulate = true;
    } else if constexpr (OP == OP_PRED_V) {
        // V[m, c] = sum_{kt = c}^{nb-1} U[m, kt] W[kt, c]      (U = X W^T, n0pad x npad; W lower triangular)
        // k tiles walked from nb-1 DOWN to c, as OP_LAUUM walks its B operand: every tile starts on the last block row of W,
        // and the triangular diagonal tile W[c, c] comes last (its zero stages are skipped like OP_TRTRI_T's)
        const int c = bid / g.p0, m = bid % g.p0;                  // p0 = row tiles of U; longest k loops (small c) first
        A0 = Ab + (size_t)m * TM * g.ldA + (size_t)(g.nb - 1) * TM; dA = -(ptrdiff_t)TM;
        B0 = Bb + (size_t)(g.nb - 1) * TM * g.ldB + (size_t)c * TM; dB = -(ptrdiff_t)TM * g.ldB;
        nkt = g.nb - c;
        Ct = Cb + (size_t)m * TM * g.ldC + (size_t)c * TM;
    } else {
        // OP_PRED_U: U[m, r] = sum_{kt = 0}^{r} X[m, kt] W[r, kt]^T    (X = scaled cross covariance, n0pad x npad)
        const int r = g.nb - 1 - bid / g.p0, m = bid % g.p0;       // p0 = row tiles of X; longest k loops (large r) first
        A0 = Ab + (size_t)m * TM * g.ldA; dA = TM;
        B0 = Bb + (size_t)r * TM * g.ldB; dB = TM;
        nkt = r + 1;
        Ct = Cb + (size_t)m * TM * g.ldC + (size_t)r * TM;
    }

    const int tid = body_tid();
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: the sub-tile origin (wm0, wn0) stays in SGPRs
    const int wm0 = (wave >> 1) * WTM, wn0 = (wave & 1) * WTN;
    typedef typename Mfma<T>::acc_t acc_t;
    acc_t acc[MIM][MIN];
    // address of accumulator element (i, j, e) in the C tile = wave-uniform part (scalar registers) + this lane's element offset
    // (byte offsets: a 128-row tile of the largest matrix spans 128 x 16384 x 8 bytes)
    const __amdgpu_buffer_rsrc_t crs = tile_rsrc(Ct);
    const unsigned cvoff = (unsigned)(Mfma<T>::lane_row(lane) * g.ldC + (lane & 15)) * (unsigned)sizeof(T);
    auto c_soff = [&](int i, int e) -> unsigned {
        return (unsigned)((wm0 + i * 16 + Mfma<T>::reg_row(e)) * g.ldC + wn0) * (unsigned)sizeof(T);
    };
    // C -= A B^T: the accumulators start from the C tile (its load overlaps the first operand loads) and the A
    // fragments are negated, so the epilogue is stores only
    constexpr bool PRELOAD_C = (OP == OP_SYRK);
#pragma unroll
    for (int i = 0; i < MIM; ++i)
#pragma unroll
        for (int j = 0; j < MIN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (PRELOAD_C) {
                    acc[i][j][e] = BufIo<T>::load(crs, cvoff + j * 16 * (unsigned)sizeof(T), c_soff(i, e));
                } else {
                    acc[i][j][e] = 0;
                }
            }

    constexpr int SPT = TM / KT;   // stages per k tile
    const int nst = nkt * SPT;
    // (measurement support: where the host passes the two clock words -- the launch that forms A^-1 = W^T W, in either tile
    // size, and the first wide trailing update of the factorisation, which is what is left to stamp where A^-1 is accumulated
    // behind the chain -- wave 0 of the first block (the longest K loop of such a launch) stamps its K loop and epilogue
    // with the shader-clock counter and the 100 MHz real-time counter, both scalar: the ratio is the clock the chip held.
    // The window is approximate: the stamps are scalar instructions the compiler may schedule a few instructions into the
    // prologue / epilogue either way)
    unsigned long long clk0 = 0, rt0 = 0;
    if constexpr (OP == OP_LAUUM || OP == OP_SYRK) {
        if (g.clk && lin == 0 && wave == 0) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
    }
    // The LAST k tile of the triangular products holds a triangular TM x TM block of W (LAUUM: W[r,r] as A, and as B too
    // on a diagonal tile; TRTRI_T: W11[cl,cl] as B; TRTRI_W: W22[rl,rl] as A; PRED_U: W[r,r] as B; PRED_V: W[c,c] as B).  In the stage that
    // covers its k rows [ks, ks + 16) a wave whose rows (columns) of that operand lie wholly on the zero side would
    // only add exact zeros: it skips the stage's fragment reads and MFMAs (one wave-uniform test per stage, nothing
    // else changes; bit-identical results: the zeros are stored zeros).  LAUUM / TRTRI_W: 24 of the 64 (wave, stage)
    // pairs of such a tile, TRTRI_T / PRED_U / PRED_V: 16.
    constexpr bool HAS_TRI = OP != OP_SYRK && OP != OP_PRED_COV && OP != OP_VR && OP != OP_VG_P && OP != OP_VG_G && OP != OP_HESS_G &&
                             OP != OP_COND_CROSS && OP != OP_COND_U;
    const int tri_first = HAS_TRI ? (nkt - 1) * SPT : nst;
    // the wave is idle in the stages [dead_lo, dead_hi) of the k loop (two scalars per wave)
    int dead_lo = nst, dead_hi = nst;
    if constexpr (OP == OP_LAUUM) { dead_lo = tri_first; dead_hi = tri_first + (tri_b && wn0 > wm0 ? wn0 : wm0) / KT; }
    else if constexpr (OP == OP_TRTRI_T || OP == OP_PRED_V) { dead_lo = tri_first; dead_hi = tri_first + wn0 / KT; }
    else if constexpr (OP == OP_TRTRI_W) dead_lo = tri_first + (wm0 + WTM) / KT;
    else if constexpr (OP == OP_PRED_U) dead_lo = tri_first + (wn0 + WTN) / KT;
    auto wave_live = [&](int sg) { return !HAS_TRI || sg < dead_lo || sg >= dead_hi; };
    constexpr bool ROWS_A = LA == MK && sizeof(T) == 8, ROWS_B = LB == MK && sizeof(T) == 8;     // (store_stage_rows)
    static_assert(TM * LDK <= KT * LD, "the row image fits the stage buffer");
    auto put_a = [&](T* S, const T (&reg)[EPT]) {
        if constexpr (ROWS_A) store_stage_rows<TM, NT>((double*)S, (const double (&)[EPT])reg, tid);
        else store_stage<T, LA, TM, NT>(S, reg, tid);
    };
    auto put_b = [&](T* S, const T (&reg)[EPT]) {
        if constexpr (ROWS_B) store_stage_rows<TM, NT>((double*)S, (const double (&)[EPT])reg, tid);
        else store_stage<T, LB, TM, NT>(S, reg, tid);
    };
    auto compute_stage = [&](int buf) {
        const T* as = As + buf * KT * LD;
        const T* bs = Bs + buf * KT * LD;
        const int l15 = lane & 15;
#pragma unroll
        for (int kk = 0; kk < KT / 4; ++kk) {
            const int krow = (kk * 4 + (lane >> 4)) * LD;
            const int kcol = kk * 4 + (lane >> 4);
            T af[MIM], bf[MIN];
#pragma unroll
            for (int i = 0; i < MIM; ++i) {
                const T v = ROWS_A ? as[(wm0 + i * 16 + l15) * LDK + kcol] : as[krow + wm0 + swz_col<T>(i * 16, l15, kk)];
                af[i] = PRELOAD_C ? -v : v;
            }
#pragma unroll
            for (int j = 0; j < MIN; ++j)
                bf[j] = ROWS_B ? bs[(wn0 + j * 16 + l15) * LDK + kcol] : bs[krow + wn0 + swz_col<T>(j * 16, l15, kk)];
#pragma unroll
            for (int i = 0; i < MIM; ++i)
#pragma unroll
                for (int j = 0; j < MIN; ++j) acc[i][j] = Mfma<T>::run(af[i], bf[j], acc[i][j]);
        }
    };
    bool done = false;
    if constexpr (TM == 64) {
        // K = 64: such a launch is one or two rounds of tiles and its time is the latency of ONE tile -- fetch all
        // four stages up front (one memory latency instead of four)
        if (nkt == 1) {
            T pa[SPT][EPT], pb[SPT][EPT];
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                load_stage<T, LA, TM, NT>(A0, g.ldA, s * KT, pa[s], tid);
                load_stage<T, LB, TM, NT>(B0, g.ldB, s * KT, pb[s], tid);
            }
#pragma unroll
            for (int s = 0; s < SPT; ++s) {
                put_a(As + (s & 1) * KT * LD, pa[s]);
                put_b(Bs + (s & 1) * KT * LD, pb[s]);
                __syncthreads();
                if (wave_live(s)) compute_stage(s & 1);
            }
            done = true;
        }
    }
    if (!done) {
        // register prefetch PF stages ahead (the loads of stage s+PF are issued while stage s is multiplied): with
        // few workgroups per CU one stage of MFMAs (~0.5 us) does not cover an HBM/L2 round trip; the 64-tile kernel,
        // whose launches are often a fraction of a round, looks a whole k tile ahead
        // Depth by register budget (128 VGPRs per lane at the occupancy the launches need): two stages everywhere since
        // round 6 -- the fp64 rank-k update, which holds its C tile in the accumulators from the start, looked ONE stage
        // ahead until the C tile moved to buffer addressing (one offset register instead of eight 64-bit row pointers) and
        // the k-contiguous operands to their row image (one fragment address instead of four): 119 registers at one stage,
        // 128 without a spill at two (profiles/r06_syrk_ab.txt: -0.09 ms per evaluation).  The hand-counted form of the loop
        // is not used for it: beside the 64 loads of the C tile the compiler spills accumulators around the loop.
        constexpr int PF = OP != OP_SYRK && TM == 64 && sizeof(T) == 4 ? 4 : 2;     // fp32 64-tile products: a whole k tile
        constexpr int NPC = EPT * (int)sizeof(T) / 16;      // 16-byte pieces per lane, operand and stage
        constexpr bool COUNTED = PF == 2 && (NPC == 1 || NPC == 2 || NPC == 4) && !PRELOAD_C;
        if constexpr (COUNTED) {
            // the hand-counted form of the loop below (see gload_piece): same stage images, same order of arithmetic
            typedef typename Piece<T>::v pc_t;
            constexpr int NL = 2 * NPC;                     // loads per register set
            pc_t qa[PF][NPC], qb[PF][NPC];
            auto put_ap = [&](T* S, const pc_t (&reg)[NPC]) {
                if constexpr (ROWS_A) store_stage_rows_p<TM, NT>((double*)S, (const Piece<double>::v (&)[NPC])reg, tid);
                else store_stage_p<T, LA, TM, NT>(S, reg, tid);
            };
            auto put_bp = [&](T* S, const pc_t (&reg)[NPC]) {
                if constexpr (ROWS_B) store_stage_rows_p<TM, NT>((double*)S, (const Piece<double>::v (&)[NPC])reg, tid);
                else store_stage_p<T, LB, TM, NT>(S, reg, tid);
            };
            const unsigned voffA = stage_lane_offset<T, LA, TM, NT>(g.ldA, tid), voffB = stage_lane_offset<T, LB, TM, NT>(g.ldB, tid);
            // NO control flow between an asm load and the wait that covers it: at a join the compiler may move a value to
            // another register, and a move placed behind the asm copies the register before the data has arrived.  The number
            // of stages is a positive multiple of SPT >= 4, so the first PF stages exist and the loop ends with exactly PF
            // stages that have nothing left to fetch.
            static_assert(SPT % PF == 0 && SPT >= 2 * PF, "stage count of a k tile");
#pragma unroll
            for (int h = 0; h < PF; ++h) {
                const int kt = h / SPT, ks = (h % SPT) * KT;
                load_stage_p<T, LA, TM, NT>(A0 + (ptrdiff_t)kt * dA, g.ldA, ks, qa[h], voffA);
                load_stage_p<T, LB, TM, NT>(B0 + (ptrdiff_t)kt * dB, g.ldB, ks, qb[h], voffB);
            }
            int s = 0;
            // main part: every stage of a pass exists and has a stage PF ahead to fetch: PF sets are outstanding whenever
            // one is stored, the oldest of them is complete at vmcnt((PF - 1) NL)
            for (; s + 2 * PF <= nst; s += PF) {
#pragma unroll
                for (int h = 0; h < PF; ++h) {
                    const int buf = (PF & 1) ? ((s + h) & 1) : (h & 1);
                    vm_wait_set<(PF - 1) * NL>(qa[h], qb[h]);
                    put_ap(As + buf * KT * LD, qa[h]);
                    put_bp(Bs + buf * KT * LD, qb[h]);
                    __syncthreads();
                    const int kt = (s + h + PF) / SPT, ks = ((s + h + PF) % SPT) * KT;
                    load_stage_p<T, LA, TM, NT>(A0 + (ptrdiff_t)kt * dA, g.ldA, ks, qa[h], voffA);
                    load_stage_p<T, LB, TM, NT>(B0 + (ptrdiff_t)kt * dB, g.ldB, ks, qb[h], voffB);
                    if (wave_live(s + h)) compute_stage(buf);
                }
            }
            // the last PF stages (s = nst - PF here): nothing left to fetch, the sets in flight are waited for together
#pragma unroll
            for (int h = 0; h < PF; ++h) {
                const int buf = (PF & 1) ? ((s + h) & 1) : (h & 1);
                vm_wait_set<0>(qa[h], qb[h]);
                put_ap(As + buf * KT * LD, qa[h]);
                put_bp(Bs + buf * KT * LD, qb[h]);
                __syncthreads();
                if (wave_live(s + h)) compute_stage(buf);
            }
            // (nothing the asm loaded is outstanding here: the last stored set was waited for with vmcnt(0))
        } else {
            T ra[PF][EPT], rb[PF][EPT];
            const unsigned uoffA = stage_lane_offset<T, LA, TM, NT>(g.ldA, tid), uoffB = stage_lane_offset<T, LB, TM, NT>(g.ldB, tid);
#pragma unroll
            for (int h = 0; h < PF; ++h) {
                if (h < nst) {
                    const int kt = h / SPT, ks = (h % SPT) * KT;
                    load_stage_u<T, LA, TM, NT>(A0 + (ptrdiff_t)kt * dA, g.ldA, ks, ra[h], uoffA);
                    load_stage_u<T, LB, TM, NT>(B0 + (ptrdiff_t)kt * dB, g.ldB, ks, rb[h], uoffB);
                }
            }
            for (int s = 0; s < nst; s += PF) {
#pragma unroll
                for (int h = 0; h < PF; ++h) {       // static register index h; LDS buffer (s + h) & 1
                    if (s + h < nst) {
                        const int buf = (PF & 1) ? ((s + h) & 1) : (h & 1);
                        put_a(As + buf * KT * LD, ra[h]);
                        put_b(Bs + buf * KT * LD, rb[h]);
                        __syncthreads();
                        if (s + h + PF < nst) {
                            const int kt = (s + h + PF) / SPT, ks = ((s + h + PF) % SPT) * KT;
                            load_stage_u<T, LA, TM, NT>(A0 + (ptrdiff_t)kt * dA, g.ldA, ks, ra[h], uoffA);
                            load_stage_u<T, LB, TM, NT>(B0 + (ptrdiff_t)kt * dB, g.ldB, ks, rb[h], uoffB);
                        }
                        if (wave_live(s + h)) compute_stage(buf);
                    }
                }
            }
        }
    }
    if constexpr (OP == OP_VR) {
        const int ct = bid % g.p1, rt = bid / g.p1;
        if (g.kern == 0) vr_epilogue<T, 0, TM, MIM, MIN>(g, acc, k, rt, ct, tid, wm0, wn0, lds);
        else if (g.kern == 1) vr_epilogue<T, 1, TM, MIM, MIN>(g, acc, k, rt, ct, tid, wm0, wn0, lds);
        else vr_epilogue<T, 2, TM, MIM, MIN>(g, acc, k, rt, ct, tid, wm0, wn0, lds);
        return;
    }
    if constexpr (OP == OP_PRED_COV) alpha = -g.theta[(size_t)k * g.p1 + g.p2];
    if constexpr (OP == OP_COND_CROSS) alpha = -g.theta[(size_t)k * g.p2 + g.p3];
#pragma unroll
    for (int mi = 0; mi < MIM; ++mi)
#pragma unroll
        for (int ni = 0; ni < MIN; ++ni)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned dvoff = cvoff + ni * 16 * (unsigned)sizeof(T), dsoff = c_soff(mi, e);
                if constexpr (OP == OP_SYRK && TM == 128) {
                    if (g.skipq && bid + g.t0 == 0 && wm0 + mi * 16 + Mfma<T>::row(lane, e) < TS && wn0 + ni * 16 + (lane & 15) < TS)
                        continue;
                }
                if constexpr (PRELOAD_C) {
                    BufIo<T>::store((T)acc[mi][ni][e], crs, dvoff, dsoff);
                } else {
                    double v = alpha * (double)acc[mi][ni][e];
                    if (accumulate) v += (double)BufIo<T>::load(crs, dvoff, dsoff);
                    BufIo<T>::store((T)v, crs, dvoff, dsoff);
                }
            }
    if constexpr (OP == OP_LAUUM || OP == OP_SYRK) {
        if (g.clk && lin == 0 && wave == 0) {
            const unsigned long long c1 = __builtin_amdgcn_s_memtime() - clk0, r1 = __builtin_amdgcn_s_memrealtime() - rt0;
            if (lane == 0) { g.clk[0] = c1; g.clk[1] = r1; }
        }
    }
    if constexpr (OP == OP_LAUUM && TM == 128) {
        // z = A^-1 b rides on the tiles of A^-1 while they are in registers (a pass over A^-1 of its own costs 0.1 ms at
        // the headline size): tile (r, c) contributes p1 = V_rc b_c to z_r and, off the diagonal, p2 = V_rc^T b_r to z_c.
        // Per lane the products over its own accumulators, then the 16 lanes of a row group (p1) / the four row groups
        // (p2) by butterflies, then the two column halves / four row quarters of the waves through LDS; fixed orders.
        if (g.part) {
            __syncthreads();                                  // the stage buffers are free now
            double* bsh = (double*)lds;                       // [0,128): b over the tile's rows, [128,256): over its columns
            double* p1s = bsh + 256;                          // [2][128]
            double* p2s = p1s + 256;                          // [4][128]
            int r, c;
            tri_decode(bid, r, c);
            const T* bk = (const T*)g.bvec + (size_t)k * g.ldC;
            if (tid < 256) bsh[tid] = (double)bk[(size_t)(tid < 128 ? r : c) * 128 + (tid & 127)];
            __syncthreads();
            const int l15 = lane & 15;
            double s2[MIN];
#pragma unroll
            for (int j = 0; j < MIN; ++j) s2[j] = 0.0;
#pragma unroll
            for (int i = 0; i < MIM; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = wm0 + i * 16 + Mfma<T>::row(lane, e);
                    const double br = bsh[row];
                    double s1 = 0.0;
#pragma unroll
                    for (int j = 0; j < MIN; ++j) {
                        const double v = (double)acc[i][j][e];
                        s1 = fma(v, bsh[128 + wn0 + j * 16 + l15], s1);
                        s2[j] = fma(v, br, s2[j]);
                    }
                    s1 += __shfl_xor(s1, 1);
                    s1 += __shfl_xor(s1, 2);
                    s1 += __shfl_xor(s1, 4);
                    s1 += __shfl_xor(s1, 8);
                    if (l15 == 0) p1s[(wave & 1) * 128 + row] = s1;
                }
#pragma unroll
            for (int j = 0; j < MIN; ++j) {
                double v = s2[j];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if ((lane >> 4) == 0) p2s[(wave >> 1) * 128 + wn0 + j * 16 + l15] = v;
            }
            __syncthreads();
            double* pt = g.part + ((size_t)k * (g.nb * (g.nb + 1) / 2) + bid) * 256;
            if (tid < 128) pt[tid] = p1s[tid] + p1s[128 + tid];
            else if (tid < 256) {
                const int cc = tid - 128;
                pt[128 + cc] = (p2s[cc] + p2s[128 + cc]) + (p2s[256 + cc] + p2s[384 + cc]);
            }
        }
    }
}

// (OP_VR: two workgroups per CU.  Its epilogue -- kernel values, exponentials and row sums beside the accumulators -- needs
// about 200 registers; at four workgroups per CU (128 registers) both dtypes spilled in it)
template <typename T, int OP, int TM, int NW>
__global__ __launch_bounds__(NW * 64, TM == 128 ? (NW == 8 ? 4 : 2) : (OP == OP_VR ? 2 : 4)) void tile_gemm(GemmArgs g) {
    __shared__ __align__(16) unsigned char lds[4 * KT * (TM + 16) * sizeof(T)];
    gemm_body<T, OP, TM, NW>(g, blockIdx.x, lds);
}

// ---------------------------------------------------------------------------------------------------
// Filler tiles (fill_sched.h): 128 x 64 outputs on 4 waves (64 x 32 per wave, 4x2 accumulators), K = nst stages of 16.
// A filler workgroup shares its launch with the diagonal-block kernel, i.e. 256 threads and two workgroups per CU; a
// 64x64 tile then leaves the MFMA pipe half idle, this shape fills it (57 KB of LDS).  Operands in either orientation
// (MK: element (m, k) at P[m ld + k];  KM: at P[k ld + m]); C = (first ? 0 : C) +- A B^T(-like) product.
// ---------------------------------------------------------------------------------------------------
using lcgp_fill::FillJob;
using lcgp_fill::FillSet;

template <typename T, int LA, int LB, bool NEG>
__device__ __forceinline__ void rect_tile(const T* __restrict__ A0, int ldA, const T* __restrict__ B0, int ldB,
                                          T* __restrict__ Ct, int ldC, int nst, bool first, unsigned char* lds) {
    constexpr int TMR = 128, TNC = 64, NT = 256, NJ_ = TNC / 32;
    constexpr int LDA = TMR + 16, LDB = TNC + 16;
    constexpr int EA = TMR * KT / NT, EB = TNC * KT / NT;
    T* As = (T*)lds;                   // [2][KT * LDA]
    T* Bs = As + 2 * KT * LDA;         // [2][KT * LDB]
    const int tid = body_tid(), lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * (TNC / 2);
    typedef typename Mfma<T>::acc_t acc_t;
    acc_t acc[4][NJ_];
    if (first) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ_; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = 0;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ_; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[i][j][e] = Ct[(size_t)(wm0 + i * 16 + Mfma<T>::row(lane, e)) * ldC + wn0 + j * 16 + (lane & 15)];
    }
    // Software pipeline over the K stages, one barrier per stage: while the MFMAs of stage s run from LDS buffer s & 1, the
    // registers of stage s + 1 are written to the other buffer (last read in stage s - 1, i.e. before the previous
    // barrier) and the global loads of stage s + 3 are issued.  A filler workgroup is alone on its SIMDs (one wave
    // each), so nothing else hides the LDS writes: issued behind the MFMAs of the same stage they cost 0.4 us per stage.
    T ra[2][EA], rb[2][EB];
    if (nst > 0) {
        load_stage<T, LA, TMR, NT>(A0, ldA, 0, ra[0], tid);
        load_stage<T, LB, TNC, NT>(B0, ldB, 0, rb[0], tid);
    }
    if (nst > 1) {
        load_stage<T, LA, TMR, NT>(A0, ldA, KT, ra[1], tid);
        load_stage<T, LB, TNC, NT>(B0, ldB, KT, rb[1], tid);
    }
    if (nst > 0) {
        store_stage<T, LA, TMR, NT>(As, ra[0], tid);
        store_stage<T, LB, TNC, NT>(Bs, rb[0], tid);
        if (nst > 2) {
            load_stage<T, LA, TMR, NT>(A0, ldA, 2 * KT, ra[0], tid);
            load_stage<T, LB, TNC, NT>(B0, ldB, 2 * KT, rb[0], tid);
        }
        __syncthreads();
    }
    for (int s = 0; s < nst; s += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (s + h < nst) {
                const T* as = As + h * KT * LDA;
                const T* bs = Bs + h * KT * LDB;
#pragma unroll
                for (int kk = 0; kk < KT / 4; ++kk) {
                    const int kr = kk * 4 + (lane >> 4);
                    T af[4], bf[NJ_];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const T v = as[kr * LDA + wm0 + swz_col<T>(i * 16, lane & 15, kk)];
                        af[i] = NEG ? -v : v;
                    }
#pragma unroll
                    for (int j = 0; j < NJ_; ++j) bf[j] = bs[kr * LDB + wn0 + swz_col<T>(j * 16, lane & 15, kk)];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < NJ_; ++j) acc[i][j] = Mfma<T>::run(af[i], bf[j], acc[i][j]);
                    if (kk == 0 && s + h + 1 < nst) {
                        // stage s + h + 1 (register set (h + 1) & 1) into the other buffer, behind the first MFMAs
                        store_stage<T, LA, TMR, NT>(As + (h ^ 1) * KT * LDA, ra[h ^ 1], tid);
                        store_stage<T, LB, TNC, NT>(Bs + (h ^ 1) * KT * LDB, rb[h ^ 1], tid);
                        if (s + h + 3 < nst) {
                            load_stage<T, LA, TMR, NT>(A0, ldA, (s + h + 3) * KT, ra[h ^ 1], tid);
                            load_stage<T, LB, TNC, NT>(B0, ldB, (s + h + 3) * KT, rb[h ^ 1], tid);
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ_; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                Ct[(size_t)(wm0 + i * 16 + Mfma<T>::row(lane, e)) * ldC + wn0 + j * 16 + (lane & 15)] = (T)acc[i][j][e];
}

// One block of a filler set: block b of the launch's filler range -> (job, component, tile) -> operands (fill_sched.h).
template <typename T>
__device__ __forceinline__ void fill_dispatch(const FillSet& fs, int b, unsigned char* lds) {
    int ji = 0;
    while (ji + 1 < fs.njobs && b >= fs.job[ji].nblk) { b -= fs.job[ji].nblk; ++ji; }
    const FillJob jb = fs.job[ji];
    const int ld = fs.npad;
    if (jb.type == lcgp_fill::FILL_TRI_T || jb.type == lcgp_fill::FILL_TRI_W) {
        GemmArgs g;
        g.sA = g.sB = g.sC = fs.mat; g.ldA = g.ldB = g.ldC = ld; g.nb = fs.nb;
        g.p0 = jb.R0; g.p1 = jb.R1; g.p2 = jb.j0; g.p3 = 0; g.q = fs.q; g.t0 = 0; g.skipq = 1;
        if (jb.type == lcgp_fill::FILL_TRI_T) {
            g.A = fs.M; g.B = fs.W; g.C = fs.V;
            gemm_body<T, OP_TRTRI_T, 64, 4>(g, b + jb.t0 * fs.q, lds);       // (a job may be split over launches)
        } else {
            g.A = fs.W; g.B = fs.V; g.C = fs.W;
            gemm_body<T, OP_TRTRI_W, 64, 4>(g, b + jb.t0 * fs.q, lds);
        }
        return;
    }
    const int k = b % fs.q;
    int t = b / fs.q + jb.t0;
    T* M = (T*)fs.M + (size_t)k * fs.mat;
    T* W = (T*)fs.W + (size_t)k * fs.mat;
    T* V = (T*)fs.V + (size_t)k * fs.mat;
    const int kb0 = jb.kb0, kb1 = jb.kb1;
    if (jb.type == lcgp_fill::FILL_SYRK) {
        // M[R, j] -= sum_k M[R, k] M[j, k]^T over the block columns [kb0, kb1)
        int j = jb.j0;
        while (t >= jb.R1 - (j >> 1)) { t -= jb.R1 - (j >> 1); ++j; }
        const int R = (j >> 1) + t;
        rect_tile<T, MK, MK, true>(M + (size_t)R * 128 * ld + (size_t)kb0 * TS, ld, M + (size_t)j * TS * ld + (size_t)kb0 * TS, ld,
                                   M + (size_t)R * 128 * ld + (size_t)j * TS, ld, (kb1 - kb0) * (TS / KT), false, lds);
    } else if (jb.type == lcgp_fill::FILL_BROW) {
        // W[R, j] = -W[R, kb0 .. ] V[kb0 .., j]: row block R of the panel's block inverse (lower triangular: k < 2R + 2)
        const int nc = jb.j1 - jb.j0;
        const int R = jb.R0 + t / nc, j = jb.j0 + t % nc;
        const int ke = kb1 < 2 * R + 2 ? kb1 : 2 * R + 2;
        rect_tile<T, MK, KM, true>(W + (size_t)R * 128 * ld + (size_t)kb0 * TS, ld, V + (size_t)kb0 * TS * ld + (size_t)j * TS, ld,
                                   W + (size_t)R * 128 * ld + (size_t)j * TS, ld, (ke - kb0) * (TS / KT), true, lds);
    } else if (jb.type == lcgp_fill::FILL_CUPD) {
        // V[R, j] (+)= M[R, kb0 ..] W[kb0 .., j]; a column inside the panel starts at its own 128-aligned block row (zeros
        // above) and is the first contribution to the tile
        const int nc = jb.j1 - jb.j0;
        const int R = jb.R0 + t / nc, j = jb.j0 + t % nc;
        const bool own = j >= kb0;
        const int ks = kb0 + (own ? ((j - kb0) & ~1) : 0);
        rect_tile<T, MK, KM, false>(M + (size_t)R * 128 * ld + (size_t)ks * TS, ld, W + (size_t)ks * TS * ld + (size_t)j * TS, ld,
                                    V + (size_t)R * 128 * ld + (size_t)j * TS, ld, (kb1 - ks) * (TS / KT), own, lds);
    } else {
        // FILL_DUPD: V[R, j] (+)= W[kb0 .., R]^T W[kb0 .., j]; a row block inside (or below) the K range starts at its own
        // block row and is written for the first time
        int R = (int)((sqrt(4.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((R + 1) * (R + 2) <= t) ++R;
        while (R * (R + 1) > t) --R;
        const int j = t - R * (R + 1);
        const bool own = 2 * R >= kb0;
        const int ks = own ? 2 * R : kb0;
        rect_tile<T, KM, KM, false>(W + (size_t)ks * TS * ld + (size_t)R * 128, ld, W + (size_t)ks * TS * ld + (size_t)j * TS, ld,
                                    V + (size_t)R * 128 * ld + (size_t)j * TS, ld, (kb1 - ks) * (TS / KT), own, lds);
    }
}

constexpr int FILL_LDS_BYTES = 2 * KT * (128 + 16 + 64 + 16) * 8;

// filler jobs on their own (what the chain launches could not carry, and the tail of the progressive inverse)
template <typename T>
__global__ __launch_bounds__(256, 2) void fill_kernel(FillSet fs) {
    __shared__ __align__(16) unsigned char lds[FILL_LDS_BYTES];
    fill_dispatch<T>(fs, blockIdx.x, lds);
}

// Heterogeneous launches.  The panel chain of the Cholesky (diagonal block -> panel TRMM -> panel update, 64 times)
// is a sequence of small dependent launches that leave most CUs idle, and two HIP streams cannot overlap them with
// the wide trailing update on this platform.  So the chain launches CARRY independent work: blocks
// beyond the chain's own are filler tiles (fill_sched.h): the previous panel's trailing update on columns the chain of
// the current panel neither reads nor writes, and the jobs of the progressive inverse.  No inter-workgroup dependency
// exists inside such a launch; stream order between launches provides all the ordering.
template <typename T>
__global__ __launch_bounds__(256, 2) void leaf_fill_kernel(T* __restrict__ M, T* __restrict__ W, size_t mat, int npad, int jb,
                                                        double* __restrict__ logdet, int* __restrict__ info,
                                                        int q, FillSet fs) {
    __shared__ __align__(16) unsigned char lds[LEAF_LDS_BYTES];
    if ((int)blockIdx.x < q) leaf_body<T>(lds, blockIdx.x, M, W, mat, npad, jb, logdet, info);
    else fill_dispatch<T>(fs, blockIdx.x - q, lds);
}

// ---------------------------------------------------------------------------------------------------
// One launch per 64-column step of the panel chain.
// The three dependent launches of a step (diagonal block -> panel TRMM -> rank-64 update of the rest of the panel)
// are re-cut so that a step needs ONE launch X_c with no dependency between its workgroups:
//   * TRMM tiles (r, c), r > c:   L[r,c] = (A[r,c] - L[r,c-1] L[c,c-1]^T) W_cc^T   -- the contribution of the
//     PREVIOUS column is applied by the tile itself, the older ones arrived through the delayed updates below;
//     a tile whose row lies inside the panel also applies  A[r,r] -= L[r,c] L[r,c]^T  to its row's diagonal tile
//     (so the panel's diagonal tiles have exactly one writer per launch);
//   * the tile (c+1, c) is "special": after the two steps above its workgroup factors and inverts the diagonal
//     block c+1 (leaf_body), which is what launch X_{c+1} needs;
//   * delayed updates, one visit per tile: the tiles (r, c+1), r > c+1, of the next column receive the columns
//     J .. c-1 in one K loop (all of them final before this launch; column c is folded into the next step's TRMM);
//   * filler tiles of the previous panel's trailing update (syrk_rect_body) as before.
// Per panel of 4 columns: 1 diagonal-block launch + 4 step launches instead of 12 launches, and the chain of a step
// is  2-3 K=64 products + one diagonal block  on a single workgroup.
// ---------------------------------------------------------------------------------------------------
struct StepArgs {
    void* M; void* W; size_t mat; int npad; int nb;
    int c, J, pe;        // this step's column, the panel [J, pe)  (64-block units)
    int diag_end;        // TRMM tiles of rows < diag_end also update their row's diagonal tile (pe, or pe + 1 when the
                         // next panel's first diagonal block is factored by the trailing-update launch)
    int q;
    int has_special;     // tile (c+1, c) continues with the diagonal block c+1  (c + 1 < pe)
    int n_trmm;          // TRMM tiles per component INCLUDING the special one: rows trmm_r0 .. trmm_r0 + n_trmm - 1
    int n_upd;           // delayed-update tiles per component: rows upd_r0 .. upd_r0 + n_upd - 1
    int trmm_r0, upd_r0; // c + 1 / c + 2 for a whole step; the persistent launch cuts a step into the rows the next diagonal
                         // blocks need and the rows below (fill_sched.h: run_interleaved)
    double* logdet; int* info;
    FillSet fs;          // filler jobs (fs.nblk blocks)
};

template <typename T>
struct Tile64 {          // 64x64 tile on 256 threads: wave (wm, wn) owns a 32x32 quadrant = 2x2 MFMA accumulators
    typedef typename Mfma<T>::acc_t acc_t;
    static constexpr int LD = TS + 16, NT = 256, EPT = TS * KT / NT, SPT = TS / KT;
    static __device__ __forceinline__ void load(acc_t (&acc)[2][2], const T* Ct, int ld, int lane, int wm0, int wn0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[i][j][e] = Ct[(size_t)(wm0 + i * 16 + Mfma<T>::row(lane, e)) * ld + wn0 + j * 16 + (lane & 15)];
    }
    static __device__ __forceinline__ void zero(acc_t (&acc)[2][2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = 0;
    }
    static __device__ __forceinline__ void store(const acc_t (&acc)[2][2], T* Ct, int ld, int lane, int wm0, int wn0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    Ct[(size_t)(wm0 + i * 16 + Mfma<T>::row(lane, e)) * ld + wn0 + j * 16 + (lane & 15)] = (T)acc[i][j][e];
    }
    // One 64x64 operand (element (m, k) at P[m * ld + k]) into registers: all four K stages at once = one memory latency
    static __device__ __forceinline__ void fetch(T (&p)[SPT][EPT], const T* P, int ld, int tid) {
#pragma unroll
        for (int s = 0; s < SPT; ++s) load_stage<T, MK, TS, NT>(P, ld, s * KT, p[s], tid);
    }
    // acc += (NEG ? -1 : 1) * A B^T from fetched operands, staged through the two LDS buffers of each
    template <bool NEG>
    static __device__ __forceinline__ void mma_regs(acc_t (&acc)[2][2], const T (&pa)[SPT][EPT], const T (&pb)[SPT][EPT],
                                                    T* lds, int tid, int lane, int wm0, int wn0) {
        T* As = lds;
        T* Bs = As + 2 * KT * LD;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            store_stage<T, MK, TS, NT>(As + (s & 1) * KT * LD, pa[s], tid);
            store_stage<T, MK, TS, NT>(Bs + (s & 1) * KT * LD, pb[s], tid);
            __syncthreads();
            const T* as = As + (s & 1) * KT * LD;
            const T* bs = Bs + (s & 1) * KT * LD;
#pragma unroll
            for (int kk = 0; kk < KT / 4; ++kk) {
                const int krow = (kk * 4 + (lane >> 4)) * LD;
                T af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const T v = as[krow + wm0 + swz_col<T>(i * 16, lane & 15, kk)];
                    af[i] = NEG ? -v : v;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = bs[krow + wn0 + swz_col<T>(j * 16, lane & 15, kk)];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = Mfma<T>::run(af[i], bf[j], acc[i][j]);
            }
        }
    }
    template <bool NEG>
    static __device__ __forceinline__ void mma(acc_t (&acc)[2][2], const T* A0, int ldA, const T* B0, int ldB, T* lds,
                                               int tid, int lane, int wm0, int wn0) {
        T pa[SPT][EPT], pb[SPT][EPT];
        fetch(pa, A0, ldA, tid);
        fetch(pb, B0, ldB, tid);
        mma_regs<NEG>(acc, pa, pb, lds, tid, lane, wm0, wn0);
    }
    // ---- products of the panel chain whose operand is a tile this workgroup has just computed: it stays on chip ----
    // The accumulator tile as a complete k-major LDS operand, F[k * LD + (m ^ (k & 15))] = tile(m, k)   (TS * LD elements).
    // The 16 contiguous lanes of a ds_write_b64 group hold 16 consecutive k of ONE row m here, i.e. 16 addresses LD
    // apart = one bank pair (16-way conflict, 1.6 us per tile -- more than the L2 round trip it is meant to replace);
    // XOR-ing the column with the low four bits of k gives the 16 lanes 16 different bank pairs, and a fragment read
    // (16 consecutive columns of one k row) only sees a permutation of its aligned group.
    static __device__ __forceinline__ void to_operand(const acc_t (&acc)[2][2], T* F, int lane, int wm0, int wn0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    F[(wn0 + j * 16 + (lane & 15)) * LD + ((wm0 + i * 16 + Mfma<T>::row(lane, e)) ^ (lane & 15))] = acc[i][j][e];
    }
    // acc += (NEG ? -1 : 1) * A B^T,  A = F (to_operand), B fetched; Bs = two staging buffers of KT * LD elements.
    // The first barrier inside also orders the writes of F.
    template <bool NEG>
    static __device__ __forceinline__ void mma_a_lds(acc_t (&acc)[2][2], const T* F, const T (&pb)[SPT][EPT], T* Bs, int tid,
                                                     int lane, int wm0, int wn0) {
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            store_stage<T, MK, TS, NT>(Bs + (s & 1) * KT * LD, pb[s], tid);
            __syncthreads();
            const T* as = F + s * KT * LD;
            const T* bs = Bs + (s & 1) * KT * LD;
#pragma unroll
            for (int kk = 0; kk < KT / 4; ++kk) {
                const int krow = (kk * 4 + (lane >> 4)) * LD;
                T af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const T v = as[krow + wm0 + i * 16 + ((lane & 15) ^ (4 * kk + (lane >> 4)))];
                    af[i] = NEG ? -v : v;
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = bs[krow + wn0 + swz_col<T>(j * 16, lane & 15, kk)];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = Mfma<T>::run(af[i], bf[j], acc[i][j]);
            }
        }
    }
    // acc += (NEG ? -1 : 1) * F^T-free form  X X^T  with X = the tile in F  (no staging, no barrier inside)
    template <bool NEG>
    static __device__ __forceinline__ void mma_ab_lds(acc_t (&acc)[2][2], const T* F, int lane, int wm0, int wn0) {
#pragma unroll
        for (int kk = 0; kk < TS / 4; ++kk) {
            const int krow = (kk * 4 + (lane >> 4)) * LD;
            T af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const T v = F[krow + wm0 + i * 16 + ((lane & 15) ^ ((4 * kk + (lane >> 4)) & 15))];
                af[i] = NEG ? -v : v;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = F[krow + wn0 + j * 16 + ((lane & 15) ^ ((4 * kk + (lane >> 4)) & 15))];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = Mfma<T>::run(af[i], bf[j], acc[i][j]);
        }
    }
};

template <typename T>
__device__ __forceinline__ void chain_step_body(const StepArgs& a, int b, unsigned char* lds) {
    typedef Tile64<T> TL;
    const int tid = body_tid(), lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int ld = a.npad;
    // block order = longest first: the special tiles (chain of the step), the filler tiles, then the short ones
    const int nspecial = a.has_special * a.q;
    int t = -1, k = 0;
    if (b < nspecial) { t = 0; k = b; }
    else if (b < nspecial + a.fs.nblk) { fill_dispatch<T>(a.fs, b - nspecial, lds); return; }
    else {
        b -= nspecial + a.fs.nblk;
        if (b < (a.n_trmm - a.has_special) * a.q) { k = b % a.q; t = b / a.q + a.has_special; }
        else b -= (a.n_trmm - a.has_special) * a.q;
    }
    if (t >= 0) {
        if (t == 0 && a.has_special) __builtin_amdgcn_s_setprio(3);   // the chain of the step shares its CU with other tiles
        const int c = a.c, r = a.trmm_r0 + t;
        T* Mk = (T*)a.M + (size_t)k * a.mat;
        const T* Wk = (const T*)a.W + (size_t)k * a.mat;
        T* Ct = Mk + (size_t)r * TS * ld + (size_t)c * TS;
        // The tile stays on chip between its products: after the previous column's contribution it goes to LDS as a
        // complete k-major operand (F), L[r,c] = tile W_cc^T reads it from there, and so does the update of the row's
        // diagonal block (X X^T with X = L[r,c]); only L[r,c] itself and the diagonal block travel to memory.  W_cc is
        // fetched before the first product, so the second one starts without a memory latency of its own.
        T* F = (T*)lds;                        // TS * LD elements (= the four staging buffers of TL::mma)
        T* Bst = F + TS * TL::LD;              // two B staging buffers behind it
        typename TL::acc_t acc[2][2];
        T pw[TL::SPT][TL::EPT];
        TL::fetch(pw, Wk + (size_t)c * TS * ld + (size_t)c * TS, ld, tid);
        TL::load(acc, Ct, ld, lane, wm0, wn0);
        if (c > a.J) {       // the previous column's contribution to this tile
            TL::template mma<true>(acc, Mk + (size_t)r * TS * ld + (size_t)(c - 1) * TS, ld,
                                   Mk + (size_t)c * TS * ld + (size_t)(c - 1) * TS, ld, (T*)lds, tid, lane, wm0, wn0);
            __syncthreads();                   // the staging buffers become F
        }
        TL::to_operand(acc, F, lane, wm0, wn0);
        TL::zero(acc);
        TL::template mma_a_lds<false>(acc, F, pw, Bst, tid, lane, wm0, wn0);
        TL::store(acc, Ct, ld, lane, wm0, wn0);         // L[r, c]
        if (r < a.diag_end) {
            T* Dt = Mk + (size_t)r * TS * ld + (size_t)r * TS;
            typename TL::acc_t dacc[2][2];
            TL::load(dacc, Dt, ld, lane, wm0, wn0);     // in flight across the barriers
            __syncthreads();                            // every read of the old F has been issued and consumed
            TL::to_operand(acc, F, lane, wm0, wn0);
            __syncthreads();
            TL::template mma_ab_lds<true>(dacc, F, lane, wm0, wn0);
            if (a.has_special && t == 0) {
                // the updated diagonal block goes to the factorisation through LDS (leaf_body's w area, which that routine
                // does not write before its first barrier); the block's L and inverse are what memory gets
                __syncthreads();
                double (*blk)[LEAF_LDT] = (double (*)[LEAF_LDT])((double*)lds + TS * LEAF_LDT);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            blk[wm0 + i * 16 + Mfma<T>::row(lane, e)][wn0 + j * 16 + (lane & 15)] = (double)dacc[i][j][e];
                __syncthreads();
                leaf_body<T, true>(lds, k, (T*)a.M, (T*)a.W, a.mat, a.npad, c + 1, a.logdet, a.info);
            } else {
                TL::store(dacc, Dt, ld, lane, wm0, wn0);
            }
        }
        return;
    }
    {
        // delayed update, one visit per tile: the tiles (r, c + 1), r > c + 1, of the NEXT column receive the columns
        // J .. c-1 in one K loop (column c itself is folded into the next step's TRMM tiles)
        k = b % a.q;
        t = b / a.q;
        const int cc = a.c + 1;
        const int r = a.upd_r0 + t;
        T* Mk = (T*)a.M + (size_t)k * a.mat;
        T* Ct = Mk + (size_t)r * TS * ld + (size_t)cc * TS;
        typename TL::acc_t acc[2][2];
        TL::load(acc, Ct, ld, lane, wm0, wn0);
        // two operand sets: the next product's tiles are in flight while the current one runs
        T pa[2][TL::SPT][TL::EPT], pb[2][TL::SPT][TL::EPT];
        const T* Ar = Mk + (size_t)r * TS * ld;
        const T* Br = Mk + (size_t)cc * TS * ld;
        TL::fetch(pa[0], Ar + (size_t)a.J * TS, ld, tid);
        TL::fetch(pb[0], Br + (size_t)a.J * TS, ld, tid);
        for (int j = a.J; j < a.c; j += 2) {
            if (j + 1 < a.c) {
                TL::fetch(pa[1], Ar + (size_t)(j + 1) * TS, ld, tid);
                TL::fetch(pb[1], Br + (size_t)(j + 1) * TS, ld, tid);
            }
            TL::template mma_regs<true>(acc, pa[0], pb[0], (T*)lds, tid, lane, wm0, wn0);
            if (j + 1 < a.c) {
                if (j + 2 < a.c) {
                    TL::fetch(pa[0], Ar + (size_t)(j + 2) * TS, ld, tid);
                    TL::fetch(pb[0], Br + (size_t)(j + 2) * TS, ld, tid);
                }
                TL::template mma_regs<true>(acc, pa[1], pb[1], (T*)lds, tid, lane, wm0, wn0);
            }
        }
        TL::store(acc, Ct, ld, lane, wm0, wn0);
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void chain_step_kernel(StepArgs a) {
    __shared__ __align__(16) unsigned char lds[LEAF_LDS_BYTES];
    chain_step_body<T>(a, blockIdx.x, lds);
}

// Trailing update of a panel that also factors the FIRST diagonal block of the next panel: the first q workgroups run
// leaf_body on that 64x64 block (the chain steps of the panel have already applied the panel to it: diag_end = pe + 1),
// the others are the tiles of the wide update (tile 0 of the 128-tile form leaves that quadrant alone; the 64-tile form
// starts at tile 1).  The next panel's chain then starts with its first step launch -- one dependent launch less per
// panel, and the diagonal block hides under the update.
template <typename T, int TM>
__global__ __launch_bounds__(256, 2) void wide_leaf_kernel(GemmArgs g, T* __restrict__ M, T* __restrict__ W, size_t mat,
                                                           int npad, int jb, double* __restrict__ logdet,
                                                           int* __restrict__ info) {
    constexpr int WIDE_LDS = 4 * KT * (TM + 16) * (int)sizeof(T);
    __shared__ __align__(16) unsigned char lds[WIDE_LDS > LEAF_LDS_BYTES ? WIDE_LDS : LEAF_LDS_BYTES];
    const int q = g.q;
    if ((int)blockIdx.x < q) {
        leaf_body<T>(lds, blockIdx.x, M, W, mat, npad, jb, logdet, info);
        return;
    }
    gemm_body<T, OP_SYRK, TM, 4>(g, blockIdx.x - q, lds);
}

// ---------------------------------------------------------------------------------------------------
// z = A^-1 b with A^-1 stored as lower 64x64 tiles, every tile read ONCE:
//   symv_tile_kernel : tile (r, c) -> p1 = V_tile b_c (64 values, belongs to z_r) and, off the diagonal,
//                      p2 = V_tile^T b_r (belongs to z_c); written to the partial buffer [tile][2][64]
//   symv_reduce_kernel: z_R = sum_{c <= R} p1(R, c) + sum_{r > R} p2(r, R)      (fixed summation order)
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void symv_tile_kernel(const T* __restrict__ V, size_t mat, int npad,
                                                        const T* __restrict__ b, double* __restrict__ part, int ntile) {
    __shared__ double vt[TS][TS + 1];
    __shared__ double red[4][TS];
    __shared__ double br[TS], bc[TS];
    const int k = blockIdx.y;
    int r, c;
    tri_decode(blockIdx.x, r, c);
    const T* Vt = V + (size_t)k * mat + (size_t)r * TS * npad + (size_t)c * TS;
    const int tid = threadIdx.x, j = tid & 63, g = tid >> 6;
    if (tid < TS) {
        br[tid] = (double)b[(size_t)k * npad + r * TS + tid];
        bc[tid] = (double)b[(size_t)k * npad + c * TS + tid];
    }
    double v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = (double)Vt[(size_t)(g * 16 + m) * npad + j];
    __syncthreads();
    double* dst = part + ((size_t)k * ntile + blockIdx.x) * 2 * TS;
    // p2[j] = sum_i V[i][j] b_r[i]: each thread sums its 16 rows, then the 4 row groups
    double s2 = 0.0;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        s2 = fma(v[m], br[g * 16 + m], s2);
        vt[g * 16 + m][j] = v[m];
    }
    red[g][j] = s2;
    __syncthreads();
    if (tid < TS) dst[TS + tid] = r == c ? 0.0 : (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    // p1[i] = sum_j V[i][j] b_c[j]: thread (i = tid & 63, g) sums columns 16 g .. 16 g + 15 from the LDS copy
    double s1 = 0.0;
#pragma unroll
    for (int m = 0; m < 16; ++m) s1 = fma(vt[j][g * 16 + m], bc[g * 16 + m], s1);
    __syncthreads();
    red[g][j] = s1;
    __syncthreads();
    if (tid < TS) dst[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

template <typename T, int TZ>
__global__ __launch_bounds__(256) void symv_reduce_kernel(const double* __restrict__ part, int ntile, int npad, int nb,
                                                          T* __restrict__ z) {
    // TZ = tile size of the partials (64: symv_tile_kernel, 128: the epilogue of the 128-tile LAUUM); nb in TZ units.
    // 256 / TZ groups of TZ threads take every NG-th term; the partial sums are combined in a fixed order
    constexpr int NG = 256 / TZ;
    __shared__ double sh[NG][TZ];
    const int k = blockIdx.y, R = blockIdx.x, i = threadIdx.x % TZ, g = threadIdx.x / TZ;
    const double* pk = part + (size_t)k * ntile * 2 * TZ;
    double s = 0.0;
    for (int c = g; c <= R; c += NG) s += pk[((size_t)(R * (R + 1) / 2 + c)) * 2 * TZ + i];
    for (int r = R + 1 + g; r < nb; r += NG) s += pk[((size_t)(r * (r + 1) / 2 + R)) * 2 * TZ + TZ + i];
    sh[g][i] = s;
    __syncthreads();
    if (g == 0) {
        double v;
        if constexpr (NG == 4) v = (sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]);
        else v = sh[0][i] + sh[1][i];
        z[(size_t)k * npad + R * TZ + i] = (T)v;
    }
}

// ---------------------------------------------------------------------------------------------------
// K5: fused gradient contraction over the lower tiles of A^-1 (HBM read once):
//   G_ij = sr_i sr_j (D/2 Ainv_ij - z_i z_j / 2),  weight 2 off the diagonal,
//   part[0..d-1] = sum w G C0 S_j^2/(1+S_j),  part[d] = sum w G C0,  part[d+1] = sum_i G_ii
// C0 and S_j are recomputed from x in LDS.  Per-tile partial sums, reduced later in fixed order.
// ---------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------
// finalize: per component, reduce the tile partials, quad = b.(b - z), pack output (gsig_a = Y[a,:].(b - z): gsig_body).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* sh /*>= 4*/, int tid) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// gsig_a = sum_i Y[a, i] (b_i - z_i): one workgroup per (output a, component); rides in the launch of the gradient
// contraction (blocks past the tiles), like b in the kernel-build launch
template <typename T>
__device__ __forceinline__ void gsig_body(int a, int k, int n, int npad, int d, int p, const T* __restrict__ Y,
                                          const T* __restrict__ b, const T* __restrict__ z, double* __restrict__ out) {
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const T* bk = b + (size_t)k * npad;
    const T* zk = z + (size_t)k * npad;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += (double)Y[(size_t)a * n + i] * ((double)bk[i] - (double)zk[i]);
    s = block_sum(s, sh, tid);
    if (tid == 0) out[(size_t)k * (d + 5 + p) + 5 + d + a] = s;
}

// float32 (CZ): the quadratic form b^T (b - z) and the noise gradient Y (b - z) cancel when A is close to the identity
// (z ~ b), and an fp32 z carries an error of 6e-8 |b| -- the same size as b - z itself in that regime (the NLL of the
// n = 16384 configuration moved by 1.6e-4 relative, enough to end an L-BFGS-B run early or late).  A z = b gives
//   b - z = D (C o s s^T) z   exactly,
// whose error is D C (error of z): small exactly where the difference cancels.  The kernel matrix is recomputed tile by
// tile here anyway, so the tiles also emit the symmetric matrix-vector partials of c = (C o s s^T) z in double:
//   cpart[tile][0][i] = sum_j Cs_ij z_j  (rows of the tile),  cpart[tile][1][j] = sum_{i != j} Cs_ij z_i  (its columns)
template <typename T, int DD, int KERN>
__global__ __launch_bounds__(256) void grad_kernel(const T* __restrict__ V, size_t mat, int n, int npad, int d, int p,
                                                   const T* __restrict__ x, const T* __restrict__ sr,
                                                   const T* __restrict__ z, const double* __restrict__ theta,
                                                   double* __restrict__ part, int ntile, const T* __restrict__ Y,
                                                   const T* __restrict__ bvec, double* __restrict__ out,
                                                   double* __restrict__ cpart) {
    constexpr bool CZ = sizeof(T) == 4;
    if ((int)blockIdx.x >= ntile) {
        gsig_body<T>(blockIdx.x - ntile, blockIdx.y, n, npad, d, p, Y, bvec, z, out);
        return;
    }
    __shared__ double xr[TS][DD + 1];
    __shared__ double xc[TS][DD + 1];
    __shared__ double zr[TS], zc[TS], srr[TS], src[TS];
    __shared__ double red[4][DD + 2];
    const int k = blockIdx.y;
    int r, c;
    tri_decode(blockIdx.x, r, c);
    const double* th = th_row(theta, d, p, k);
    const double D = th[d + 2];
    const int tid = threadIdx.x;
    // scaled inputs of the tile's rows and columns; the dimensions d .. DD-1 of the instantiation are zero-filled, so the
    // loops below run over DD without a test (a zero distance leaves every product and sum unchanged)
    for (int e = tid; e < TS * DD; e += 256) {
        int i = e / DD, j = e - i * DD;
        int gi = r * TS + i, gj = c * TS + i;
        xr[i][j] = (j < d && gi < n) ? (double)x[(size_t)gi * d + j] / th[j] : 0.0;
        xc[i][j] = (j < d && gj < n) ? (double)x[(size_t)gj * d + j] / th[j] : 0.0;
    }
    if (tid < TS) {
        int gi = r * TS + tid, gj = c * TS + tid;
        zr[tid] = (double)z[(size_t)k * npad + gi];
        zc[tid] = (double)z[(size_t)k * npad + gj];
        srr[tid] = (sr && gi < n) ? (double)sr[gi] : 1.0;
        src[tid] = (sr && gj < n) ? (double)sr[gj] : 1.0;
    }
    __syncthreads();
    double acc[DD + 2];
#pragma unroll
    for (int e = 0; e < DD + 2; ++e) acc[e] = 0.0;
    double cz1[CZ ? 8 : 1], cz2[CZ ? 2 : 1];      // c partials: the thread's 8 rows (over its 2 columns), its 2 columns (over its rows)
    if constexpr (CZ) {
#pragma unroll
        for (int m = 0; m < 8; ++m) cz1[m] = 0.0;
        cz2[0] = cz2[1] = 0.0;
    }
    const double scale_c = th[d], nt_c = th[d + 1] / (1.0 + th[d + 1]);
    const T* Vk = V + (size_t)k * mat;
    // thread = two adjacent columns (one 16-byte load per row in fp64) x 8 rows: two independent chains per load
    const int j0 = (tid & 31) * 2;
    typedef T pair_t __attribute__((ext_vector_type(2)));
    // all eight rows of the thread are requested up front (the padded matrix has every row of the tile), and the scaled
    // inputs of its two columns stay in registers when the instantiation is narrow enough
    pair_t avs[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
        avs[m] = *(const pair_t*)(Vk + (size_t)(r * TS + (tid >> 5) * 8 + m) * npad + c * TS + j0);
    constexpr bool HOIST = DD <= 10;
    double xcv[2][HOIST ? DD : 1];
    if constexpr (HOIST) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int jj = 0; jj < DD; ++jj) xcv[h][jj] = xc[j0 + h][jj];
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = (tid >> 5) * 8 + m;
        const int gi = r * TS + i;
        if (gi >= n) continue;
        const pair_t av = avs[m];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = j0 + h;
            const int gj = c * TS + j;
            if (gj >= n || gj > gi) continue;
            const double ainv = (double)av[h];
            const double wgt = gi == gj ? 1.0 : 2.0;
            const double G = wgt * srr[i] * src[j] * (0.5 * D * ainv - 0.5 * zr[i] * zc[j]);
            // C0 S_j^2 / (1 + S_j) = exp(-sum S) S_j^2 prod_{i != j} (1 + S_i): prefix / suffix products, no division
            double sv[DD], pre[DD];
            double prod = 1.0, ssum = 0.0;
#pragma unroll
            for (int jj = 0; jj < DD; ++jj) {
                double xcj;
                if constexpr (HOIST) xcj = xcv[h][jj]; else xcj = xc[j][jj];
                if constexpr (KERN == 0) {
                    const double s = fabs(xr[i][jj] - xcj);
                    sv[jj] = s;
                    pre[jj] = prod;
                    prod = fma(prod, s, prod);
                    ssum -= s;
                } else if constexpr (KERN == 1) {   // squared exponential: dC0/d ell_j = C0 S_j^2 / ell_j, no polynomial factor
                    const double s = xr[i][jj] - xcj;
                    sv[jj] = s;
                    ssum = fma(-0.5 * s, s, ssum);
                } else {            // Matern-5/2: as 3/2 with the factor f(S) = 1 + S + S^2 / 3
                    static_assert(KERN == 2, "unknown covariance kernel id");
                    const double s = fabs(xr[i][jj] - xcj);
                    sv[jj] = s;
                    pre[jj] = prod;
                    prod = fma(prod, m52_fm1(s), prod);
                    ssum -= s;
                }
            }
            // C0 = 0 where its exponential underflows, and the polynomial beside it may have overflowed (inf x 0): no contribution.
            // (Only the widest instantiation can get there: (1 + S)^16 stays finite for every S below 1e19; the Matern-5/2
            // factor grows with S^2, so there the same holds up to 8 dimensions.)
            if constexpr (DD > (KERN == 2 ? 8 : 16)) { if (ssum < exp_floor<double>()) continue; }
            const double ex = exp_nonpos(ssum);
            const double ge = G * ex;
            if constexpr (CZ) {
                const double cs = srr[i] * src[j] * scale_c * ((1.0 - nt_c) * (ex * prod) + (gi == gj ? nt_c : 0.0));
                cz1[m] = fma(cs, zc[j], cz1[m]);
                if (gi != gj) cz2[h] = fma(cs, zr[i], cz2[h]);
            }
            double suf = 1.0;
#pragma unroll
            for (int jj = DD - 1; jj >= 0; --jj) {
                if constexpr (KERN == 0) {
                    acc[jj] = fma(ge * (sv[jj] * sv[jj]), pre[jj] * suf, acc[jj]);
                    suf = fma(suf, sv[jj], suf);
                } else if constexpr (KERN == 1) {
                    acc[jj] = fma(ge, sv[jj] * sv[jj], acc[jj]);
                } else {            // C0 S^2 (1 + S) / (3 f(S_j)) = exp(-sum S) m52_wl(S_j) prod_{i != j} f(S_i)
                    static_assert(KERN == 2, "unknown covariance kernel id");
                    acc[jj] = fma(ge * m52_wl(sv[jj]), pre[jj] * suf, acc[jj]);
                    suf = fma(suf, m52_fm1(sv[jj]), suf);
                }
            }
            acc[DD] = fma(ge, prod, acc[DD]);
            if (gi == gj) acc[DD + 1] += G;
        }
    }
    // deterministic block reduction: wave butterfly, then 4 waves through LDS
#pragma unroll
    for (int e = 0; e < DD + 2; ++e) {
        double v = acc[e];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        acc[e] = v;
    }
    if ((tid & 63) == 0)
#pragma unroll
        for (int e = 0; e < DD + 2; ++e) red[tid >> 6][e] = acc[e];
    __syncthreads();
    if (tid < d + 2) {
        const int e = tid < d ? tid : (DD + tid - d);
        double* dst = part + ((size_t)k * ntile + blockIdx.x) * (DMAX + 2);       // (stride of the narrow kernels: d <= 32)
        dst[tid] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    }
    if constexpr (CZ) {
        // rows: the 32 lanes of a half wave share the thread's 8 rows (butterfly); columns: the 8 row groups through LDS
        __shared__ double c2s[8][TS];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            double v = cz1[m];
            for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
            cz1[m] = v;
        }
        c2s[tid >> 5][j0] = cz2[0];
        c2s[tid >> 5][j0 + 1] = cz2[1];
        __syncthreads();
        double* dst = cpart + ((size_t)k * ntile + blockIdx.x) * 2 * TS;
        if ((tid & 31) == 0) {
#pragma unroll
            for (int m = 0; m < 8; ++m) dst[(tid >> 5) * 8 + m] = cz1[m];
        }
        if (tid < TS)
            dst[TS + tid] = ((c2s[0][tid] + c2s[1][tid]) + (c2s[2][tid] + c2s[3][tid])) +
                            ((c2s[4][tid] + c2s[5][tid]) + (c2s[6][tid] + c2s[7][tid]));
    }
}

// The same contraction for d > 32 (the reference's kernel loops over any number of input dimensions, covmat.py:35-42;
// its examples stop at 10): the dimensions are staged in LDS 32 at a time.  A first sweep over the chunks gives every
// element its total product and exponent; then one sweep per chunk with the dimension as the OUTER loop,
//   sum_ij G_ij e^{-sum S} S_j^2 prod_{i != j} (1 + S_i)  =  sum_ij ge_ij S_j^2 (prod_ij / (1 + S_j)),
// one accumulator at a time (per-thread accumulators for all d dimensions would not fit the register file; the division
// replaces the prefix/suffix products of the narrow kernels).  Per-tile partial sums have stride d + 2.
template <typename T, int KERN>
__global__ __launch_bounds__(256) void grad_kernel_wide(const T* __restrict__ V, size_t mat, int n, int npad, int d, int p,
                                                        const T* __restrict__ x, const T* __restrict__ sr,
                                                        const T* __restrict__ z, const double* __restrict__ theta,
                                                        double* __restrict__ part, int ntile, const T* __restrict__ Y,
                                                        const T* __restrict__ bvec, double* __restrict__ out,
                                                        double* __restrict__ cpart) {
    constexpr bool CZ = sizeof(T) == 4;
    if ((int)blockIdx.x >= ntile) {
        gsig_body<T>(blockIdx.x - ntile, blockIdx.y, n, npad, d, p, Y, bvec, z, out);
        return;
    }
    __shared__ double xr[TS][DMAX + 1];
    __shared__ double xc[TS][DMAX + 1];
    __shared__ double zr[TS], zc[TS], srr[TS], src[TS];
    __shared__ double red[4][DWIDE + 2];
    const int k = blockIdx.y;
    int r, c;
    tri_decode(blockIdx.x, r, c);
    const double* th = th_row(theta, d, p, k);
    const double D = th[d + 2];
    const double scale_c = th[d], nt_c = th[d + 1] / (1.0 + th[d + 1]);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TS) {
        int gi = r * TS + tid, gj = c * TS + tid;
        zr[tid] = (double)z[(size_t)k * npad + gi];
        zc[tid] = (double)z[(size_t)k * npad + gj];
        srr[tid] = (sr && gi < n) ? (double)sr[gi] : 1.0;
        src[tid] = (sr && gj < n) ? (double)sr[gj] : 1.0;
    }
    const T* Vk = V + (size_t)k * mat;
    const int j0 = (tid & 31) * 2;
    typedef T pair_t __attribute__((ext_vector_type(2)));
    pair_t avs[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
        avs[m] = *(const pair_t*)(Vk + (size_t)(r * TS + (tid >> 5) * 8 + m) * npad + c * TS + j0);
    auto stage = [&](int d0) {       // scaled inputs of the dimensions d0 .. d0 + 31 (zero beyond d)
        __syncthreads();
        for (int e = tid; e < TS * DMAX; e += 256) {
            int i = e / DMAX, jj = e - i * DMAX;
            int gi = r * TS + i, gj = c * TS + i;
            xr[i][jj] = (d0 + jj < d && gi < n) ? (double)x[(size_t)gi * d + d0 + jj] / th[d0 + jj] : 0.0;
            xc[i][jj] = (d0 + jj < d && gj < n) ? (double)x[(size_t)gj * d + d0 + jj] / th[d0 + jj] : 0.0;
        }
        __syncthreads();
    };
    double prodT[16], geT[16];          // element e = 2 m + h: total product, then G e^{-sum S}
#pragma unroll
    for (int e = 0; e < 16; ++e) { prodT[e] = 1.0; geT[e] = 0.0; }
    for (int d0 = 0; d0 < d; d0 += DMAX) {
        stage(d0);
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = (tid >> 5) * 8 + m, j = j0 + h;
                double pr = prodT[2 * m + h], ss = geT[2 * m + h];
                for (int jj = 0; jj < DMAX; ++jj) {
                    if constexpr (KERN == 0) {
                        const double s = fabs(xr[i][jj] - xc[j][jj]);
                        pr = fma(pr, s, pr);
                        ss -= s;
                    } else if constexpr (KERN == 1) {
                        const double s = xr[i][jj] - xc[j][jj];
                        ss = fma(-0.5 * s, s, ss);
                    } else {
                        static_assert(KERN == 2, "unknown covariance kernel id");
                        const double s = fabs(xr[i][jj] - xc[j][jj]);
                        pr = fma(pr, m52_fm1(s), pr);
                        ss -= s;
                    }
                }
                prodT[2 * m + h] = pr;
                geT[2 * m + h] = ss;
            }
    }
    double a_scale = 0.0, a_nug = 0.0;
    double cz1[CZ ? 8 : 1], cz2[CZ ? 2 : 1];
    if constexpr (CZ) {
#pragma unroll
        for (int m = 0; m < 8; ++m) cz1[m] = 0.0;
        cz2[0] = cz2[1] = 0.0;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = (tid >> 5) * 8 + m, j = j0 + h;
            const int gi = r * TS + i, gj = c * TS + j;
            double ge = 0.0;
            if (gi < n && gj < n && gj <= gi) {
                const double wgt = gi == gj ? 1.0 : 2.0;
                const double G = wgt * srr[i] * src[j] * (0.5 * D * (double)avs[m][h] - 0.5 * zr[i] * zc[j]);
                const bool zero = geT[2 * m + h] < exp_floor<double>();       // C0 = 0 (its polynomial may be inf)
                if (zero) prodT[2 * m + h] = 0.0;
                const double ex = zero ? 0.0 : exp_nonpos(geT[2 * m + h]);
                ge = G * ex;
                a_scale = fma(ge, prodT[2 * m + h], a_scale);
                if (gi == gj) a_nug += G;
                if constexpr (CZ) {
                    const double cs = srr[i] * src[j] * scale_c * ((1.0 - nt_c) * (ex * prodT[2 * m + h]) + (gi == gj ? nt_c : 0.0));
                    cz1[m] = fma(cs, zc[j], cz1[m]);
                    if (gi != gj) cz2[h] = fma(cs, zr[i], cz2[h]);
                }
            } else {
                // not part of the sum (padding, the upper half of a diagonal tile): its weight ge is zero, but its product may
                // have overflowed, and 0 x inf in the sweep below would be a NaN (Matern-5/2 at collapsed lengthscales gets
                // there from about 27 dimensions on, Matern-3/2 from about 52)
                prodT[2 * m + h] = 0.0;
            }
            geT[2 * m + h] = ge;
        }
    auto wave_sum = [&](double v) {
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        return v;
    };
    for (int d0 = 0; d0 < d; d0 += DMAX) {
        stage(d0);
        const int dc = d - d0 < DMAX ? d - d0 : DMAX;
        for (int jj = 0; jj < dc; ++jj) {
            double a = 0.0;
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const double s = fabs(xr[(tid >> 5) * 8 + m][jj] - xc[j0 + h][jj]);
                    if constexpr (KERN == 0) a = fma(geT[2 * m + h] * (s * s), prodT[2 * m + h] / (1.0 + s), a);
                    else if constexpr (KERN == 1) a = fma(geT[2 * m + h], s * s, a);
                    else {
                        static_assert(KERN == 2, "unknown covariance kernel id");
                        a = fma(geT[2 * m + h] * m52_wl(s), prodT[2 * m + h] / (1.0 + m52_fm1(s)), a);
                    }
                }
            a = wave_sum(a);
            if (lane == 0) red[wave][d0 + jj] = a;
        }
    }
    a_scale = wave_sum(a_scale);
    a_nug = wave_sum(a_nug);
    if (lane == 0) { red[wave][d] = a_scale; red[wave][d + 1] = a_nug; }
    __syncthreads();
    if (tid < d + 2) {
        double* dst = part + ((size_t)k * ntile + blockIdx.x) * (d + 2);
        dst[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
    if constexpr (CZ) {
        __shared__ double c2s[8][TS];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            double v = cz1[m];
            for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
            cz1[m] = v;
        }
        c2s[tid >> 5][j0] = cz2[0];
        c2s[tid >> 5][j0 + 1] = cz2[1];
        __syncthreads();
        double* dst = cpart + ((size_t)k * ntile + blockIdx.x) * 2 * TS;
        if ((tid & 31) == 0) {
#pragma unroll
            for (int m = 0; m < 8; ++m) dst[(tid >> 5) * 8 + m] = cz1[m];
        }
        if (tid < TS)
            dst[TS + tid] = ((c2s[0][tid] + c2s[1][tid]) + (c2s[2][tid] + c2s[3][tid])) +
                            ((c2s[4][tid] + c2s[5][tid]) + (c2s[6][tid] + c2s[7][tid]));
    }
}

// c_R = sum_{c <= R} cpart(R, c)[0] + sum_{r >= R} cpart(r, R)[1]   (the diagonal tile's column part holds its strictly lower
// elements only), fixed order; one workgroup per 64-row block and component
__global__ __launch_bounds__(256) void cvec_reduce_kernel(const double* __restrict__ cpart, int ntile, int npad, int nb,
                                                          double* __restrict__ c) {
    __shared__ double sh[4][TS];
    const int k = blockIdx.y, R = blockIdx.x, i = threadIdx.x & 63, g = threadIdx.x >> 6;
    const double* pk = cpart + (size_t)k * ntile * 2 * TS;
    double s = 0.0;
    for (int cc = g; cc <= R; cc += 4) s += pk[((size_t)(R * (R + 1) / 2 + cc)) * 2 * TS + i];
    for (int r = R + g; r < nb; r += 4) s += pk[((size_t)(r * (r + 1) / 2 + R)) * 2 * TS + TS + i];
    sh[g][i] = s;
    __syncthreads();
    if (g == 0) c[(size_t)k * npad + R * TS + i] = (sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]);
}

// float32: gsig_a = D sum_i Y[a, i] c_i   (= sum_i Y[a, i] (b_i - z_i) without the cancellation)
template <typename T>
__global__ __launch_bounds__(256) void gsig_c_kernel(int n, int npad, int d, int p, const T* __restrict__ Y,
                                                     const double* __restrict__ c, const double* __restrict__ theta,
                                                     double* __restrict__ out) {
    __shared__ double sh[4];
    const int a = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const double* ck = c + (size_t)k * npad;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += (double)Y[(size_t)a * n + i] * ck[i];
    s = block_sum(s, sh, tid);
    if (tid == 0) out[(size_t)k * (d + 5 + p) + 5 + d + a] = th_row(theta, d, p, k)[d + 2] * s;
}


template <typename T>
__global__ __launch_bounds__(256) void finalize_kernel(int n, int npad, int d, int p, int ntile,
                                                       const T* __restrict__ Y, const T* __restrict__ b,
                                                       const T* __restrict__ z, const double* __restrict__ part,
                                                       const double* __restrict__ logdet, const int* __restrict__ info,
                                                       const double* __restrict__ theta, double* __restrict__ out,
                                                       const double* __restrict__ cvec /*float32: (C o s s^T) z, else null*/) {
    __shared__ double sh[4];
    __shared__ double grp[256];
    __shared__ double sums[DWIDE + 2];
    const int pstride = (d > DMAX ? d : DMAX) + 2;       // doubles per tile in `part` (grad_kernel / grad_kernel_wide)
    const int k = blockIdx.x;
    const int tid = threadIdx.x;
    const double* th = th_row(theta, d, p, k);
    double* o = out + (size_t)k * (d + 5 + p);
    const T* bk = b + (size_t)k * npad;
    const T* zk = z + (size_t)k * npad;
    // tile partials: thread = (entry e = tid % ne, group g = tid / ne) sums its entry over the tiles g, g + ng, ...;
    // entry e then adds its ng group sums in a fixed order (one pass over the partials, deterministic)
    const int ne = d + 2, ng = 256 / ne;
    const int e = tid % ne, g = tid / ne;
    double acc = 0.0;
    if (g < ng) {
        // four independent chains (the loads of one chain would otherwise wait for each other), combined in a fixed order
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        const double* pk = part + (size_t)k * ntile * pstride + e;
        int t = g;
        for (; t + 3 * ng < ntile; t += 4 * ng) {
            a0 += pk[(size_t)t * pstride];
            a1 += pk[(size_t)(t + ng) * pstride];
            a2 += pk[(size_t)(t + 2 * ng) * pstride];
            a3 += pk[(size_t)(t + 3 * ng) * pstride];
        }
        for (; t < ntile; t += ng) a0 += pk[(size_t)t * pstride];
        acc = (a0 + a1) + (a2 + a3);
    }
    grp[tid] = acc;
    double v = 0.0;
    if (cvec) {
        // b^T (b - z) = D b^T (C o s s^T) z: no cancellation (see grad_kernel)
        const double* ck = cvec + (size_t)k * npad;
#pragma unroll 4
        for (int i = tid; i < n; i += 256) v += (double)bk[i] * ck[i];
        v *= th[d + 2];
    } else {
#pragma unroll 4
        for (int i = tid; i < n; i += 256) v += (double)bk[i] * ((double)bk[i] - (double)zk[i]);
    }
    __syncthreads();
    if (tid < ne) {
        double s = 0.0;
        for (int gg = 0; gg < ng; ++gg) s += grp[gg * ne + tid];
        sums[tid] = s;
    }
    const double quad = block_sum(v, sh, tid);          // (its barriers also publish sums[])
    const double scale = th[d], nug = th[d + 1];
    const double nt = nug / (1.0 + nug);
    if (tid == 0) {
        o[0] = logdet[k];
        o[1] = quad;
        o[2] = (double)info[k];
        for (int j = 0; j < d; ++j) o[3 + j] = scale * (1.0 - nt) / th[j] * sums[j];
        o[3 + d] = (1.0 - nt) * sums[d] + nt * sums[d + 1];
        o[4 + d] = scale * (sums[d + 1] - sums[d]) / ((1.0 + nug) * (1.0 + nug));
    }
}


// small helpers ----------------------------------------------------------------------------------------
__global__ void zero_stats_kernel(double* logdet, int* info, int q) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) { logdet[i] = 0.0; info[i] = 0; }
}

__global__ void copy_stats_kernel(const double* logdet, const int* info, double* ld_out, int* info_out, int q) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) { if (ld_out) ld_out[i] = logdet[i]; if (info_out) info_out[i] = info[i]; }
}

template <typename T>
__global__ void fetch_kernel(const T* __restrict__ src, int npad, int n, T* __restrict__ dst) {
    int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= n) return;
    dst[(size_t)i * n + j] = j <= i ? src[(size_t)i * npad + j] : src[(size_t)j * npad + i];
}

// ghat[k, m] = sum_i X_k[m, i] z_k[i] ;  gvar[k, m] = scale_k - D_k * sum_i U_k[m, i]^2        (one wave per row m)
template <typename T>
__global__ __launch_bounds__(64) void pred_reduce_kernel(const T* __restrict__ X, const T* __restrict__ U, size_t slab, size_t uslab, int ld,
                                                         int n, const T* __restrict__ z, int npad,
                                                         const double* __restrict__ theta, int tw, int d, int ldo,
                                                         double* __restrict__ ghat, double* __restrict__ gvar,
                                                         int ldu = 0 /*row length of U; 0 = ld*/) {
    const int m = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], D = th[d + 2];
    const T* Xr = X + (size_t)k * slab + (size_t)m * ld;
    const T* Ur = U + (size_t)k * uslab + (size_t)m * (ldu ? ldu : ld);
    const T* zk = z + (size_t)k * npad;
    double s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double u = (double)Ur[i];
        s1 += (double)Xr[i] * (double)zk[i];
        s2 += u * u;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
    if (lane == 0) { ghat[(size_t)k * ldo + m] = s1; gvar[(size_t)k * ldo + m] = scale - D * s2; }
}

// pred_reduce_kernel with the prior of a box average: scale_k (1 - nt_k) prod_{l in the row's mask} I2[k, l] (ascending l;
// the nugget is white noise, its average over a set of positive measure vanishes); a row with an empty mask keeps scale_k
// and is bitwise pred_reduce_kernel's
template <typename T>
__global__ __launch_bounds__(64) void marg_reduce_kernel(const T* __restrict__ X, const T* __restrict__ U, size_t slab, int ld, int n,
                                                         const T* __restrict__ z, int npad, const double* __restrict__ theta, int tw,
                                                         int d, const unsigned char* __restrict__ mask,
                                                         const double* __restrict__ i2, int ldo, double* __restrict__ ghat,
                                                         double* __restrict__ gvar) {
    const int m = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const T* Xr = X + (size_t)k * slab + (size_t)m * ld;
    const T* Ur = U + (size_t)k * slab + (size_t)m * ld;
    const T* zk = z + (size_t)k * npad;
    double s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double u = (double)Ur[i];
        s1 += (double)Xr[i] * (double)zk[i];
        s2 += u * u;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
    if (lane == 0) {
        double pr = scale * (1.0 - nug / (1.0 + nug));
        bool any = false;
        for (int l = 0; l < d; ++l)
            if (mask[(size_t)m * d + l]) { pr *= i2[(size_t)k * d + l]; any = true; }
        const double prior = any ? pr : scale;
        ghat[(size_t)k * ldo + m] = s1;
        gvar[(size_t)k * ldo + m] = prior - D * s2;
    }
}

// the widened row [U_r | T_r] of pass row r (lcgp_condition_predict_marginal, ref_out): ref[k, 0 .. npad) = U_k[r, :],
// ref[k, npad .. npad + mpad) = T_k[r, :] (mpad = 0 without a view).  grid ((npad + mpad) / 256 rounded up, q)
template <typename T>
__global__ __launch_bounds__(256) void marg_refrow_kernel(const T* __restrict__ U, size_t slab, int npad, const T* __restrict__ Tm,
                                                          size_t cslab, int mpad, int r, T* __restrict__ ref) {
    const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (j >= npad + mpad) return;
    ref[(size_t)k * (npad + mpad) + j] = j < npad ? U[(size_t)k * slab + (size_t)r * npad + j]
                                                  : Tm[(size_t)k * cslab + (size_t)r * mpad + (j - npad)];
}

// gcov[k, i] = prior_k(i, r) - D_k U_k[i, :] . U_r - T_k[i, :] . T_r: the posterior covariance of the box average of row i with
// that of a reference row r given as its widened row ref = [U_r | T_r] (marg_refrow_kernel), its values xr and its mask mr.
// prior_k(i, r) = scale_k (1 - nt_k) prod_l f_l in ascending l, f_l = kappa(|x0_il - xr_l| / ell_kl) where both rows keep l,
// the box average of kappa at the kept value where one row integrates l, I2[k, l] where both do; no nugget term (the
// continuous surface).  One wave per row: the lanes stride the n columns of U and then the m columns of T (m = 0: no view),
// butterfly sums as in pred_reduce_kernel and cond_reduce_kernel; lane 0 forms the prior.  An entry of x0 or xr under its
// row's mask is never loaded.
template <typename T, int KERN>
__global__ __launch_bounds__(64) void marg_refcov_kernel(const T* __restrict__ U, size_t slab, int npad, int n,
                                                         const T* __restrict__ Tm, size_t cslab, int mpad, int m,
                                                         const T* __restrict__ ref, const double* __restrict__ theta, int tw,
                                                         int d, const T* __restrict__ x0, const unsigned char* __restrict__ mask,
                                                         const T* __restrict__ xr, const unsigned char* __restrict__ mr,
                                                         const double* __restrict__ box, const double* __restrict__ i2, int ldo,
                                                         double* __restrict__ gcov) {
    const int i = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    const T* Ui = U + (size_t)k * slab + (size_t)i * npad;
    const T* rf = ref + (size_t)k * (npad + mpad);
    double s1 = 0.0, s2 = 0.0;
    for (int j = lane; j < n; j += 64) s1 += (double)Ui[j] * (double)rf[j];
    if (m > 0) {
        const T* Ti = Tm + (size_t)k * cslab + (size_t)i * mpad;
        for (int j = lane; j < m; j += 64) s2 += (double)Ti[j] * (double)rf[npad + j];
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
    if (lane == 0) {
        const double scale = th[d], nug = th[d + 1], D = th[d + 2];
        double pr = scale * (1.0 - nug / (1.0 + nug));
        for (int l = 0; l < d; ++l) {
            const bool mi = mask[(size_t)i * d + l] != 0, mj = mr[l] != 0;
            const double ell = th[l];
            double f;
            if (mi && mj) {
                f = i2[(size_t)k * d + l];
            } else if (mi || mj) {
                const double xv = mi ? (double)xr[l] : (double)x0[(size_t)i * d + l];
                f = marg_I1<KERN>(xv, box[l], box[d + l], ell);
            } else {
                const double u = fabs((double)x0[(size_t)i * d + l] - (double)xr[l]) / ell;
                if constexpr (KERN == 0) f = (1.0 + u) * exp(-u);
                else if constexpr (KERN == 1) f = exp(-0.5 * u * u);
                else f = (1.0 + u + u * u / 3.0) * exp(-u);
            }
            pr *= f;
        }
        gcov[(size_t)k * ldo + i] = pr - D * s1 - s2;
    }
}

// ---------------------------------------------------------------------------------------------------
// K7: input gradients of the prediction.  For local component k, new input i (standardised) and dimension l:
//   dghat[k, i, l] =        sum_j dc_l(i, j) sr_j z_k[j]
//   dgvar[k, i, l] = -2 D_k sum_j dc_l(i, j) sr_j V_k[i, j],      V_k = X_k A_k^-1 = U_k W_k   (OP_PRED_V)
//   dc_l = -c0 s_l / (ell_l (1 + |s_l|))  (Matern-3/2),   -c0 s_l / ell_l  (SE),   s_l = (x0_il - x_jl) / ell_l,
//          -c0 s_l (1 + |s_l|) / (ell_l (3 + 3 |s_l| + s_l^2))  (Matern-5/2)
// with c0 = scale (1 - nug / (1 + nug)) C0: the nugget term has no derivative (the gradient of the continuous surface).
// The scaled distances and c0 are recomputed in registers as cross_kernel forms them; the n0 x n x d derivative tensor is
// never written.  One workgroup per (32 rows of x0, component, chunk of DD dimensions): lane & 31 = row, the 8 half-waves
// take every 8th training input of a stage of JT.  Accumulation in double (also for float32 inputs), per lane in ascending
// j; the 8 slices are then summed in a fixed order -- no atomics: bitwise reproducible, independent of q_local.
// DD < 32: d <= DD, the row of x0 held in registers.  DD = 32 serves every d in (16, 126]: c0 over all d from LDS, the
// derivative for the 32 dimensions of chunk blockIdx.z (2 DD accumulators per lane, never 2 d).
constexpr int PG_ROWS = 32, PG_SL = 8;
// ZMAT (lcgp_variance_reduction_grad): z is a matrix laid out as V is (row i0 + i of slab k, row length npad), not the vector z_k.
// MEAN (lcgp_predict_gradcov): dghat alone, by the same operations in the same order; V and dgvar are not touched.
// COND (lcgp_condition_predict_grad): the contraction runs over a SECOND segment of columns behind the training inputs, the m
// conditioning inputs xn of a view -- weight 1 instead of sr_j, w in place of z, R (rows mpad long) in place of V, the factor
// -2 in place of -2 D (D rides on the weights of the first segment) -- and z is the view's z' in double.  Same stages, same
// lane / slice / wave order; per lane the training inputs in ascending j, then the conditioning inputs in ascending j.
// COND + MEAN (lcgp_condition_predict_gradcov): dghat' alone over both segments; V', R and dgvar are not touched.
// COND + ZMAT (lcgp_condition_vr_grad): both segments carry a matrix in the place of z -- z (rows npad long, beside V) over
// the training inputs with the weight D sr_j, zn (rows mpad long, laid out as R is) over the conditioning inputs with the
// weight 1; zd and wv are not read.
template <typename T>
struct PgradCond {
    const double* zd;           // z' (q x npad doubles)
    const T* xn; int m;         // the conditioning inputs (m x d)
    const double* wv; int mpad; // w = L_S^-T v (q x mpad doubles)
    const T* R; size_t rslab;   // R = T L_S^-1 (q slabs of rows mpad long)
};

template <typename T, int DD, int KERN, bool ZMAT, bool MEAN, bool COND>
__device__ __forceinline__ void pgrad_body(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                           const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                           int tw, const T* __restrict__ z, int npad, const T* __restrict__ V,
                                           size_t slab, int ldo, double* __restrict__ dghat, double* __restrict__ dgvar,
                                           const PgradCond<T>& cs, const T* __restrict__ zn = nullptr) {
    static_assert(!ZMAT || !MEAN, "the mean-only contraction carries the vector z");
    constexpr bool WIDE = DD == DMAX;
    constexpr int JT = WIDE ? 16 : 32;                  // training inputs per LDS stage
    constexpr int XW = WIDE ? DWIDE + 3 : DD + 1;       // odd row length: the per-row reads of x0sh hit distinct banks;
                                                        // >= l0 + DD for every chunk (zeros beyond d)
    __shared__ double x0sh[PG_ROWS][XW];
    __shared__ double xsh[JT][XW];
    __shared__ double vsh[MEAN ? 1 : PG_ROWS][JT + 1];
    __shared__ double zsh[ZMAT ? PG_ROWS : 1][JT + 1];
    __shared__ double wz[JT], wsr[JT];
    __shared__ double th[DWIDE + 3];
    __shared__ double red[2][4][PG_ROWS];
    const int k = blockIdx.y, i0 = blockIdx.x * PG_ROWS, l0 = WIDE ? blockIdx.z * DMAX : 0;
    const int tid = threadIdx.x, r = tid & 31, sl = tid >> 5;
    for (int e = tid; e < d + 3; e += 256) th[e] = theta[(size_t)k * tw + e];
    __syncthreads();
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double c_off = scale * (1.0 - nug / (1.0 + nug));
    for (int e = tid; e < PG_ROWS * XW; e += 256) {
        const int i = e / XW, m = e - i * XW;
        x0sh[i][m] = (i0 + i < n0 && m < d) ? (double)x0[(size_t)(i0 + i) * d + m] / th[m] : 0.0;
    }
    const T* zk = z + (size_t)k * (ZMAT ? slab : (size_t)npad);
    const T* Vk = V + (size_t)k * slab;
    double am[DD], av[DD];
#pragma unroll
    for (int l = 0; l < DD; ++l) { am[l] = 0.0; av[l] = 0.0; }
    double xi[WIDE ? 1 : DD];
    __syncthreads();
    if constexpr (!WIDE) {
#pragma unroll
        for (int m = 0; m < DD; ++m) xi[m] = x0sh[r][m];
    }
    // (COND: the stages of the second segment follow those of the first, whose last stage may be short)
    const int n1 = (n + JT - 1) / JT * JT, jend = COND ? n1 + (cs.m + JT - 1) / JT * JT : n;
    for (int j0 = 0; j0 < jend; j0 += JT) {
        if (j0 > 0) __syncthreads();                    // every slice is done with the previous stage
        const bool seg2 = COND && j0 >= n1;
        const int jb = seg2 ? j0 - n1 : j0;             // first input of the stage within its segment
        const T* xs = seg2 ? cs.xn : x;
        const int ns = seg2 ? cs.m : n;
        for (int e = tid; e < JT * XW; e += 256) {
            const int jj = e / XW, m = e - jj * XW;
            xsh[jj][m] = (jb + jj < ns && m < d) ? (double)xs[(size_t)(jb + jj) * d + m] / th[m] : 0.0;
        }
        for (int e = tid; e < PG_ROWS * JT; e += 256) {
            const int i = e / JT, jj = e - i * JT;
            if constexpr (COND) {
                const bool in = i0 + i < n0 && jb + jj < ns;
                if constexpr (!MEAN)
                    vsh[i][jj] = !in ? 0.0 : seg2 ? (double)cs.R[(size_t)k * cs.rslab + (size_t)(i0 + i) * cs.mpad + jb + jj]
                                                  : (double)Vk[(size_t)(i0 + i) * npad + jb + jj];
                if constexpr (ZMAT)
                    zsh[i][jj] = !in ? 0.0 : seg2 ? (double)zn[(size_t)k * cs.rslab + (size_t)(i0 + i) * cs.mpad + jb + jj]
                                                  : (double)zk[(size_t)(i0 + i) * npad + jb + jj];
            } else if constexpr (!MEAN) vsh[i][jj] = (i0 + i < n0 && j0 + jj < n) ? (double)Vk[(size_t)(i0 + i) * npad + j0 + jj] : 0.0;
            if constexpr (ZMAT && !COND) zsh[i][jj] = (i0 + i < n0 && j0 + jj < n) ? (double)zk[(size_t)(i0 + i) * npad + j0 + jj] : 0.0;
        }
        if (tid < JT) {
            const int j = jb + tid;
            if constexpr (COND) {
                const double s = j < ns ? (seg2 ? 1.0 : (sr ? (double)sr[j] : 1.0)) : 0.0;
                wsr[tid] = seg2 ? s : s * D;
                if constexpr (ZMAT) wz[tid] = seg2 ? s : s * D;
                else wz[tid] = j < ns ? s * (seg2 ? cs.wv[(size_t)k * cs.mpad + j] : cs.zd[(size_t)k * npad + j]) : 0.0;
            } else {
                const double s = j < n ? (sr ? (double)sr[j] : 1.0) : 0.0;      // (inputs beyond n weigh zero)
                wsr[tid] = s;
                if constexpr (ZMAT) wz[tid] = s;
                else wz[tid] = j < n ? s * (double)zk[j] : 0.0;
            }
        }
        __syncthreads();
        for (int jj = sl; jj < JT; jj += PG_SL) {
            double poly = 1.0, ssum = 0.0;
            auto acc_c0 = [&](double df) {
                if constexpr (KERN == 0) {
                    const double sd = fabs(df);
                    poly *= 1.0 + sd;
                    ssum -= sd;
                } else if constexpr (KERN == 1) {
                    ssum = fma(-0.5 * df, df, ssum);
                } else {
                    static_assert(KERN == 2, "unknown covariance kernel id");
                    const double sd = fabs(df);
                    poly = fma(poly, m52_fm1(sd), poly);
                    ssum -= sd;
                }
            };
            if constexpr (WIDE) {
                for (int m = 0; m < d; ++m) acc_c0(x0sh[r][m] - xsh[jj][m]);
            } else {
#pragma unroll
                for (int m = 0; m < DD; ++m) acc_c0(xi[m] - xsh[jj][m]);
            }
            const double c0 = c_off * kern_c0<KERN>(poly, ssum);
            const double a = ZMAT ? c0 * wz[jj] * zsh[r][jj] : c0 * wz[jj], b = MEAN ? 0.0 : c0 * wsr[jj] * vsh[r][jj];
#pragma unroll
            for (int l = 0; l < DD; ++l) {
                const double s = WIDE ? x0sh[r][l0 + l] - xsh[jj][l0 + l] : xi[l] - xsh[jj][l];
                double h;
                if constexpr (KERN == 0) h = s * fast_rcp(1.0 + fabs(s));
                else if constexpr (KERN == 1) h = s;
                else {              // m52_wx(s) = s (1 + |s|) / (3 + 3 |s| + s^2)
                    static_assert(KERN == 2, "unknown covariance kernel id");
                    const double sa = fabs(s);
                    h = fma(s, sa, s) * fast_rcp(fma(sa, sa + 3.0, 3.0));
                }
                am[l] = fma(a, h, am[l]);
                if constexpr (!MEAN) av[l] = fma(b, h, av[l]);
            }
        }
    }
    // slices 2w and 2w + 1 share wave w (lanes r, r + 32), then the four waves through LDS: a fixed order
    const int wave = tid >> 6, i = i0 + r;
    const size_t orow = (size_t)k * ldo * d + (size_t)i * d;
#pragma unroll
    for (int l = 0; l < DD; ++l) {
        const double sm = am[l] + __shfl_xor(am[l], 32), sv = av[l] + __shfl_xor(av[l], 32);
        if ((tid & 63) < 32) { red[0][wave][r] = sm; red[1][wave][r] = sv; }
        __syncthreads();
        if (tid < PG_ROWS && i < n0 && l0 + l < d) {
            const double tm = (red[0][0][r] + red[0][1][r]) + (red[0][2][r] + red[0][3][r]);
            const double tv = (red[1][0][r] + red[1][1][r]) + (red[1][2][r] + red[1][3][r]);
            dghat[orow + l0 + l] = -tm / th[l0 + l];
            if constexpr (MEAN) (void)tv;
            else if constexpr (COND) dgvar[orow + l0 + l] = 2.0 * tv / th[l0 + l];      // (D rode on the first segment's weights)
            else dgvar[orow + l0 + l] = 2.0 * D * tv / th[l0 + l];
        }
        __syncthreads();
    }
}

template <typename T, int DD, int KERN, bool ZMAT = false, bool MEAN = false>
__global__ __launch_bounds__(256) void pgrad_kernel(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                                    const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                                    int tw, const T* __restrict__ z, int npad, const T* __restrict__ V,
                                                    size_t slab, int ldo, double* __restrict__ dghat, double* __restrict__ dgvar) {
    pgrad_body<T, DD, KERN, ZMAT, MEAN, false>(x0, n0, x, sr, n, d, theta, tw, z, npad, V, slab, ldo, dghat, dgvar, PgradCond<T>{});
}

// the contraction of lcgp_condition_predict_grad over the n training inputs and the m conditioning inputs of a view
template <typename T, int DD, int KERN>
__global__ __launch_bounds__(256) void pgrad_cond_kernel(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                                         const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                                         int tw, int npad, const T* __restrict__ V, size_t slab, int ldo,
                                                         double* __restrict__ dghat, double* __restrict__ dgvar, PgradCond<T> cs) {
    pgrad_body<T, DD, KERN, false, false, true>(x0, n0, x, sr, n, d, theta, tw, (const T*)nullptr, npad, V, slab, ldo, dghat, dgvar, cs);
}

// its MEAN instance (lcgp_condition_predict_gradcov): dghat' alone, by the same operations in the same order; V', R and dgvar
// are not touched
template <typename T, int DD, int KERN>
__global__ __launch_bounds__(256) void pgrad_cond_mean_kernel(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                                              const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                                              int tw, int npad, int ldo, double* __restrict__ dghat, PgradCond<T> cs) {
    pgrad_body<T, DD, KERN, false, true, true>(x0, n0, x, sr, n, d, theta, tw, (const T*)nullptr, npad, (const T*)nullptr, (size_t)0,
                                               ldo, dghat, (double*)nullptr, cs);
}

// the contraction of lcgp_condition_vr_grad over the n + m columns with a matrix in the place of z in both segments: z beside V
// (slabs `slab` apart, rows npad long), zn beside cs.R (slabs cs.rslab apart, rows cs.mpad long)
template <typename T, int DD, int KERN>
__global__ __launch_bounds__(256) void pgrad_cond_mat_kernel(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                                             const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                                             int tw, const T* __restrict__ z, int npad, const T* __restrict__ V,
                                                             size_t slab, int ldo, double* __restrict__ dghat,
                                                             double* __restrict__ dgvar, PgradCond<T> cs, const T* __restrict__ zn) {
    pgrad_body<T, DD, KERN, true, false, true>(x0, n0, x, sr, n, d, theta, tw, z, npad, V, slab, ldo, dghat, dgvar, cs, zn);
}

// ---------------------------------------------------------------------------------------------------
// host-side drivers (enqueue only)
// ---------------------------------------------------------------------------------------------------
#define CHECK_LAUNCH(what)                                  \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return fail(what, e__);      \
    } while (0)

// f(std::integral_constant<int, KERN>{}) for the covariance kernel id w.kern (0 = Matern-3/2, 1 = squared exponential,
// 2 = Matern-5/2; validated at the C ABI)
template <typename F>
inline void for_kern(int kern, F&& f) {
    if (kern == 0) f(std::integral_constant<int, 0>{});
    else if (kern == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}

// f(std::integral_constant<int, DD>{}) for the smallest input-dimension bound DD >= d the narrow kernels are built for
// (DMAX beyond 16)
template <typename F>
inline void for_dim(int d, F&& f) {
    if (d <= 2) f(std::integral_constant<int, 2>{});
    else if (d <= 4) f(std::integral_constant<int, 4>{});
    else if (d <= 6) f(std::integral_constant<int, 6>{});
    else if (d <= 10) f(std::integral_constant<int, 10>{});
    else if (d <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, DMAX>{});
}

template <typename T>
int do_build(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const void* Y = nullptr) {
    // with Y (the NLL path) the launch also computes b_k = Y^T psi_k into the workspace (extra blocks past the tiles) and
    // zeroes the log-determinant and status words of the components
    dim3 grid(w.ntile_lower + (Y ? (w.npad + 255) / 256 : 0), w.q);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((build_kernel<T, decltype(dd)::value, decltype(kern)::value>), grid, dim3(256), 0, st,
                               (T*)(w.base + w.off_M), w.mat, w.n, w.npad, w.d, w.p, (const T*)x, (const T*)sr, theta, w.ntile_lower,
                               (const T*)Y, (T*)(w.base + w.off_b), Y ? (double*)(w.base + w.off_logdet) : nullptr,
                               Y ? (int*)(w.base + w.off_info) : nullptr);
        });
    });
    CHECK_LAUNCH("build_kernel");
    return 0;
}

template <typename T, int OP, int TM = TS>
int launch_gemm(hipStream_t st, const GemmArgs& g, int ntiles, int q) {
    if (ntiles <= 0) return 0;
    // 128x128 tiles: eight waves (32x64 each, 128 registers, four waves per SIMD) for the long products of the inverse; FOUR
    // waves (64x64 each, 233 registers, two per SIMD, still two workgroups per CU) for the rank-256 update, whose 16-stage
    // tiles spend relatively more time at their barriers: half as many waves to synchronise, twice the MFMAs between two
    // barriers, half the fragment reads per MFMA (profiles/r06_syrk_ab.txt: 1294 -> 1242 us per evaluation; the long products
    // lose on four waves: A^-1 2.79 -> 2.83 ms)
    constexpr int NW = TM == 128 ? (OP == OP_SYRK ? 4 : 8) : 4;
    GemmArgs h = g;
    h.q = q;
    h.t0 = 0;
    h.skipq = 0;
    hipLaunchKernelGGL((tile_gemm<T, OP, TM, NW>), dim3((unsigned)ntiles * q), dim3(NW * 64), 0, st, h);
    CHECK_LAUNCH("tile_gemm");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Schedule parameters.  They travel with each call (lcgp_sched in the header; NULL = lcgp_sched_default):
// the library keeps no mutable state.  Results do not depend on them beyond rounding.
// ---------------------------------------------------------------------------------------------------
inline lcgp_sched default_sched() {
    lcgp_sched s;
    s.outer_blocks = 0;            // 0 = automatic: 4 (fp64) / 8 (fp32) 64-blocks per outer Cholesky panel
    s.syrk_small_tiles = 3000;     // below this many 128x128 tiles (x components) a trailing update runs on 64x64 tiles (2000 until
                                   // round 6: with two prefetch stages and the row image the 64-tile update caught up with the 128-tile one)
    s.trtri_small_tiles = 4200;    // the same switch for the whole triangular inverse ...
    s.lauum_small_tiles = 2048;    // ... and for A^-1 = W^T W
    s.trtri_level_small = 600;     // a single level of the triangular inverse below this many 128x128 tiles: 64x64 tiles
    s.fill_leaf = 248;             // filler blocks (128x64 tiles) carried by a diagonal-block launch
    s.fill_step = 248;             // ... and by a chain-step launch that ends in a diagonal block
    s.leaf_in_wide = 2048;         // a trailing update of at most this many 64x64 tiles also factors the next diagonal block
    s.progressive_tiles = 600;     // L^-1 and A^-1 formed behind the chain up to this many 128x128 lower tiles x components
                                   // (n = 4096: one component per rank; measured 2.72 -> 2.55 ms there, slower from two on)
    s.progressive_far = 1;         // ... with the far columns of the trailing updates still riding on the chain
    s.progressive_lauum = 48;      // ... and A^-1 = W^T W accumulated behind the chain as well up to this many 64-blocks per side
                                   // (n = 2048: 1.12 -> 0.98 ms; at n = 4096 its tail is one ragged launch of long K loops
                                   // that loses to the one-launch W^T W: 2.54 vs 2.43 ms)
    s.pair_tiles = 4000;           // paired panels: one K = 2 ob update of the columns between the second panel and the far ones
    return s;
}

inline int check_sched(const lcgp_sched& s) {
    if (s.outer_blocks < 0 || s.outer_blocks > 64) return bad("sched.outer_blocks must be in [0, 64]");
    if (s.syrk_small_tiles < 0 || s.trtri_small_tiles < 0 || s.lauum_small_tiles < 0 || s.trtri_level_small < 0 ||
        s.fill_leaf < 0 || s.fill_step < 0 || s.leaf_in_wide < 0 || s.progressive_tiles < 0 || s.progressive_lauum < 0 ||
        s.pair_tiles < 0)
        return bad("sched fields must be >= 0");
    return 0;
}

using lcgp_fill::trapezoid_tiles;

// launches the filler set on its own
template <typename T>
int launch_fill(hipStream_t st, const FillSet& fs) {
    if (fs.nblk <= 0) return 0;
    hipLaunchKernelGGL((fill_kernel<T>), dim3((unsigned)fs.nblk), dim3(256), 0, st, fs);
    CHECK_LAUNCH("fill_kernel");
    return 0;
}

// trailing update with the panel [J, pe) of the tile columns [c_lo, c_hi) (64-block units, all rows below)
template <typename T>
int potrf_trailing(hipStream_t st, const Ws& w, int J, int pe, int c_lo, int c_hi, bool tiles128, bool with_leaf,
                   unsigned long long* clk = nullptr) {
    if (c_lo >= c_hi) return 0;
    T* M = (T*)(w.base + w.off_M);
    GemmArgs g;
    g.sA = g.sB = g.sC = w.mat; g.ldA = g.ldB = g.ldC = w.npad;
    g.A = M; g.B = M; g.C = M;
    g.clk = clk;
    // 128x128 tiles when the panel boundaries are 128-aligned AND the launch has enough of them to fill the chip (the
    // plan decides); a launch with few tiles is bounded by the duration of one tile, which is 4x shorter on 64x64 tiles
    if (tiles128) {
        g.nb = w.nb / 2; g.p0 = J / 2; g.p1 = pe / 2; g.p2 = c_lo / 2; g.p3 = c_hi / 2;
        const int nt = trapezoid_tiles(w.nb / 2, c_lo / 2, c_hi / 2);
        if (with_leaf) {
            g.q = w.q; g.t0 = 0; g.skipq = 1;
            hipLaunchKernelGGL((wide_leaf_kernel<T, 128>), dim3((unsigned)(nt + 1) * w.q), dim3(256), 0, st, g, M,
                               (T*)(w.base + w.off_W), w.mat, w.npad, c_lo, (double*)(w.base + w.off_logdet),
                               (int*)(w.base + w.off_info));
            CHECK_LAUNCH("wide_leaf_kernel");
            return 0;
        }
        return launch_gemm<T, OP_SYRK, 128>(st, g, nt, w.q);
    }
    g.nb = w.nb; g.p0 = J; g.p1 = pe; g.p2 = c_lo; g.p3 = c_hi;
    const int nt = trapezoid_tiles(w.nb, c_lo, c_hi);
    if (with_leaf) {
        // tile 0 = the diagonal block itself: it belongs to the special workgroups (the chain steps of the panel have
        // already applied the panel to it)
        g.q = w.q; g.t0 = 1; g.skipq = 0;
        hipLaunchKernelGGL((wide_leaf_kernel<T, 64>), dim3((unsigned)nt * w.q), dim3(256), 0, st, g, M,
                           (T*)(w.base + w.off_W), w.mat, w.npad, c_lo, (double*)(w.base + w.off_logdet),
                           (int*)(w.base + w.off_info));
        CHECK_LAUNCH("wide_leaf_kernel");
        return 0;
    }
    return launch_gemm<T, OP_SYRK>(st, g, nt, w.q);
}

// ---- the plan of a factorisation as a caller-owned, position-independent block of bytes (lcgp_plan_build) ----
// header | Launch[nlaunch].  It depends on (dtype, n, q_local, with_inverse, sched) only, so a caller builds it once and
// passes it with every evaluation: no planning in the evaluation loop.
constexpr unsigned PLAN_MAGIC = 0x4c43504cu;
struct PlanHeader {
    unsigned magic;
    int version;
    int dtype, n, nb, q, with_inverse;
    int nlaunch;
    int inverse_done;          // what the plan leaves behind the factorisation: 0 = L, 1 = and L^-1, 2 = and A^-1
    int reserved;              // (zero; the plan is host-only: nothing in it depends on the device)
    lcgp_sched sched;
    size_t off_launch, bytes;
};

inline lcgp_fill::PlanParams plan_params(int dtype, int nb, int q, bool with_inverse, const lcgp_sched& sc, int* inverse_done) {
    lcgp_fill::PlanParams pp;
    pp.nb = nb; pp.q = q;
    pp.ob = sc.outer_blocks < 1 ? (dtype == LCGP_F32 ? 8 : 4) : sc.outer_blocks;
    pp.syrk_small_tiles = sc.syrk_small_tiles; pp.fill_leaf = sc.fill_leaf; pp.fill_step = sc.fill_step;
    pp.leaf_in_wide = sc.leaf_in_wide;
    bool prog = false;
    if (with_inverse && sc.progressive_tiles > 0 && pp.ob >= 2 && (pp.ob & (pp.ob - 1)) == 0) {
        const int nb2 = nb / 2;
        prog = (long long)q * (nb2 * (nb2 + 1) / 2) <= sc.progressive_tiles;
    }
    pp.progressive = prog;
    pp.far_rides = !(pp.progressive && sc.progressive_far == 0);
    pp.with_dupd = nb <= sc.progressive_lauum;
    pp.pair_tiles = sc.pair_tiles;
    if (inverse_done) *inverse_done = pp.progressive ? (pp.with_dupd ? 2 : 1) : 0;
    return pp;
}

// builds the plan into `out` (NULL: only the size is computed) or into `vec` (resized); returns the bytes, 0 on failure
inline size_t make_plan(int dtype, int n, int q, bool with_inverse, const lcgp_sched& sc, void* out,
                        std::vector<char>* vec = nullptr) {
    const int npad = round_up(n, 2 * TS), nb = npad / TS;
    int inverse_done = 0;
    lcgp_fill::Planner plan(plan_params(dtype, nb, q, with_inverse, sc, &inverse_done));
    plan.run();
    if (plan.failed) { bad("internal: the filler queue did not drain"); return 0; }
    PlanHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = PLAN_MAGIC; h.version = LCGP_VERSION;
    h.dtype = dtype; h.n = n; h.nb = nb; h.q = q; h.with_inverse = with_inverse ? 1 : 0;
    h.nlaunch = (int)plan.launches.size();
    h.inverse_done = inverse_done;
    h.sched = sc;
    h.off_launch = (sizeof(PlanHeader) + 255) & ~size_t(255);
    h.bytes = (h.off_launch + sizeof(lcgp_fill::Launch) * h.nlaunch + 255) & ~size_t(255);
    if (vec) { vec->resize(h.bytes); out = vec->data(); }
    if (out) {
        memset(out, 0, h.bytes);
        memcpy(out, &h, sizeof(h));
        memcpy((char*)out + h.off_launch, plan.launches.data(), sizeof(lcgp_fill::Launch) * h.nlaunch);
    }
    return h.bytes;
}

inline int check_plan(const void* plan_host, int dtype, int n, int q, bool with_inverse) {
    const PlanHeader* h = (const PlanHeader*)plan_host;
    if (h->magic != PLAN_MAGIC || h->version != LCGP_VERSION) return bad("plan: not a plan of this library version");
    if (h->dtype != dtype || h->n != n || h->q != q || h->with_inverse != (with_inverse ? 1 : 0))
        return bad("plan: built for another (dtype, n, q_local, with_inverse)");
    return 0;
}

// Two-level right-looking Cholesky.  Outer panels of `ob` 64-blocks: inside a panel every 64-column step is ONE launch
// (chain_step_kernel) that only touches the panel's block column and the rest of the panel; the trailing matrix is read
// and written once per outer panel with K = 64 ob.  The trailing update of panel J is split by columns into one wide
// launch (the columns of panel J+1 and as many more as do not fit below) and its right-most columns, which the chain
// launches of panel J+1 carry as filler tiles -- the chain leaves >= 97 % of the CUs idle, and a second HIP stream
// cannot fill them on this platform.  The launch sequence is PLANNED first (fill_sched.h: Planner, host
// only, replayed on the CPU by tests/test_fill_sched.py through tests/native/dump_plan.cpp) -- by the caller, once
// (lcgp_plan_build), or here per call when no plan is passed -- and then enqueued launch by launch.
template <typename T>
int do_potrf(hipStream_t st, const Ws& w, const lcgp_sched& sc, bool stats_zeroed = false, bool with_inverse = false,
             int* inverse_done = nullptr /* 0 = nothing, 1 = L^-1, 2 = L^-1 and A^-1 */, const void* plan_host = nullptr) {
    T* M = (T*)(w.base + w.off_M);
    T* W = (T*)(w.base + w.off_W);
    double* logdet = (double*)(w.base + w.off_logdet);
    int* info = (int*)(w.base + w.off_info);
    if (!stats_zeroed) {       // (the NLL path's kernel-build launch has done it)
        hipLaunchKernelGGL(zero_stats_kernel, dim3((w.q + 63) / 64), dim3(64), 0, st, logdet, info, w.q);
        CHECK_LAUNCH("zero_stats");
    }
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    std::vector<char> local;
    if (!plan_host) {
        if (!make_plan(dtype, w.n, w.q, with_inverse, sc, nullptr, &local)) return -1;
        plan_host = local.data();
    }
    const PlanHeader* h = (const PlanHeader*)plan_host;
    if (inverse_done) *inverse_done = h->inverse_done;
    const lcgp_fill::Launch* launches = (const lcgp_fill::Launch*)((const char*)plan_host + h->off_launch);
    const int nlaunch = h->nlaunch;
    bool first_trail = true;
    for (int li = 0; li < nlaunch; ++li) {
        const lcgp_fill::Launch& l = launches[li];
        FillSet fs = l.fs;
        fs.M = w.base + w.off_M; fs.W = w.base + w.off_W; fs.V = w.base + w.off_V;
        fs.mat = w.mat; fs.npad = w.npad; fs.nb = w.nb; fs.q = w.q;
        int rc = 0;
        switch (l.kind) {
            case lcgp_fill::L_LEAF:
                if (fs.nblk > 0)
                    hipLaunchKernelGGL((leaf_fill_kernel<T>), dim3(w.q + fs.nblk), dim3(256), 0, st, M, W, w.mat, w.npad, l.J,
                                       logdet, info, w.q, fs);
                else
                    hipLaunchKernelGGL((leaf_kernel<T>), dim3(w.q), dim3(256), 0, st, M, W, w.mat, w.npad, l.J, logdet, info);
                CHECK_LAUNCH("leaf_kernel");
                break;
            case lcgp_fill::L_STEP: {
                StepArgs a;
                a.M = M; a.W = W; a.mat = w.mat; a.npad = w.npad; a.nb = w.nb;
                a.c = l.c; a.J = l.J; a.pe = l.pe; a.q = w.q;
                a.diag_end = l.diag_end; a.has_special = l.has_special; a.n_trmm = l.n_trmm; a.n_upd = l.n_upd;
                a.trmm_r0 = l.c + 1;
                a.upd_r0 = l.c + 2;
                a.logdet = logdet; a.info = info;
                a.fs = fs;
                const long nblk = (long)(a.n_trmm + a.n_upd) * w.q + fs.nblk;
                hipLaunchKernelGGL((chain_step_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, st, a);
                CHECK_LAUNCH("chain_step_kernel");
                break;
            }
            case lcgp_fill::L_TRAIL:
                // (the first trailing update -- the widest -- leaves the clock words of lcgp_lauum_clock; a later A^-1 launch
                // overwrites them)
                rc = potrf_trailing<T>(st, w, l.J, l.pe, l.c_lo, l.c_hi, l.tiles128 != 0, l.with_leaf != 0,
                                       first_trail ? (unsigned long long*)(w.base + w.off_clock) : nullptr);
                first_trail = false;
                break;
            default:
                rc = launch_fill<T>(st, fs);
        }
        if (rc) return rc;
    }
    return 0;
}

// With few components in flight the 128x128 launches of the inverse are bounded by their LONGEST tile (one tile with
// K = 4096 keeps a CU busy for ~0.5 ms while the rest of the chip idles): below a threshold of 128-tiles per launch
// the same products run on 64x64 tiles (4x more, 4x shorter tiles).
inline bool use_small_tiles(const Ws& w, int threshold) {
    const int nb2 = w.nb / 2;
    return (long long)w.q * (nb2 * (nb2 + 1) / 2) < threshold;
}

template <typename T, int TM>
int trtri_level(hipStream_t st, const Ws& w, int mb) {      // one level: pairs of blocks of mb tiles (TM units)
    GemmArgs g;
    g.sA = g.sB = g.sC = w.mat; g.ldA = g.ldB = g.ldC = w.npad; g.p2 = g.p3 = 0;
    const int nbt = w.npad / TM;
    g.nb = nbt;
    const int pairs = (nbt + 2 * mb - 1) / (2 * mb);
    g.p0 = mb; g.p1 = pairs;
    g.A = (T*)(w.base + w.off_M); g.B = (T*)(w.base + w.off_W); g.C = (T*)(w.base + w.off_V);
    int rc = launch_gemm<T, OP_TRTRI_T, TM>(st, g, pairs * mb * mb, w.q);
    if (rc) return rc;
    g.A = (T*)(w.base + w.off_W); g.B = (T*)(w.base + w.off_V); g.C = (T*)(w.base + w.off_W);
    return launch_gemm<T, OP_TRTRI_W, TM>(st, g, pairs * mb * mb, w.q);
}

template <typename T>
int do_trtri(hipStream_t st, const Ws& w, const lcgp_sched& sc) {
    const bool all_small = use_small_tiles(w, sc.trtri_small_tiles);
    // levels in 64-block units: mb64 = 1 joins pairs of 64-blocks (always 64x64 tiles); a further level works on 128x128
    // tiles unless the whole inverse or this level is too small to fill the chip with them
    for (int mb64 = 1; mb64 < w.nb; mb64 *= 2) {
        bool small = all_small || mb64 == 1;
        if (!small) {
            const int mb = mb64 / 2, nbt = w.npad / 128;
            const long long tiles = (long long)((nbt + 2 * mb - 1) / (2 * mb)) * mb * mb * w.q;
            small = tiles < sc.trtri_level_small;
        }
        const int rc = small ? trtri_level<T, 64>(st, w, mb64) : trtri_level<T, 128>(st, w, mb64 / 2);
        if (rc) return rc;
    }
    return 0;
}

template <typename T>
int do_lauum(hipStream_t st, const Ws& w, const lcgp_sched& sc, bool* z_partials = nullptr) {
    // z_partials: the caller also wants z = A^-1 b (b in the workspace).  On 128-tiles the launch leaves the per-tile
    // partial products in the workspace (epilogue of gemm_body) and sets *z_partials; on 64-tiles it does not.
    GemmArgs g;
    g.sA = g.sB = g.sC = w.mat; g.ldA = g.ldB = g.ldC = w.npad; g.p0 = g.p1 = g.p2 = g.p3 = 0;
    g.A = (T*)(w.base + w.off_W); g.B = g.A; g.C = (T*)(w.base + w.off_V);
    if (z_partials) *z_partials = false;
    g.clk = (unsigned long long*)(w.base + w.off_clock);      // (either tile size stamps its first block: lcgp_lauum_clock)
    if (use_small_tiles(w, sc.lauum_small_tiles)) {
        g.nb = w.nb;
        return launch_gemm<T, OP_LAUUM, 64>(st, g, w.nb * (w.nb + 1) / 2, w.q);
    }
    const int nb2 = w.nb / 2;
    g.nb = nb2;
    // the epilogue runs in every 128-tile launch, also when only A^-1 is asked for (lcgp_lauum / lcgp_potri: b in the
    // workspace may then be stale and the partials are never read): one launch shape to measure and to maintain
    g.bvec = w.base + w.off_b;
    g.part = (double*)(w.base + w.off_part);
    if (z_partials) *z_partials = true;
    return launch_gemm<T, OP_LAUUM, 128>(st, g, nb2 * (nb2 + 1) / 2, w.q);
}

template <typename T>
int do_potri(hipStream_t st, const Ws& w, const lcgp_sched& sc, bool* z_partials = nullptr) {
    int rc = do_trtri<T>(st, w, sc);
    if (rc) return rc;
    return do_lauum<T>(st, w, sc, z_partials);
}

template <typename T>
int do_nll_grad(hipStream_t st, const Ws& w, const lcgp_sched& sc, const void* x, const void* Y, const void* sr,
                const double* theta, double* out, const void* plan_host) {
    int rc = do_build<T>(st, w, x, sr, theta, Y);
    if (rc) return rc;
    T* b = (T*)(w.base + w.off_b);
    T* z = (T*)(w.base + w.off_z);
    int inverse_done = 0;          // what the progressive inverse has left behind the factorisation: 1 = L^-1, 2 = and A^-1
    rc = do_potrf<T>(st, w, sc, true, true, &inverse_done, plan_host);
    if (rc) return rc;
    bool z_partials = false;       // z = A^-1 b: per-tile partials from the 128-tile LAUUM's epilogue, or a pass of its own
    if (inverse_done == 0) rc = do_potri<T>(st, w, sc, &z_partials);
    else if (inverse_done == 1) rc = do_lauum<T>(st, w, sc, &z_partials);
    if (rc) return rc;
    if (z_partials) {
        const int nb2 = w.nb / 2;
        hipLaunchKernelGGL((symv_reduce_kernel<T, 128>), dim3(nb2, w.q), dim3(256), 0, st,
                           (const double*)(w.base + w.off_part), nb2 * (nb2 + 1) / 2, w.npad, nb2, z);
    } else {
        hipLaunchKernelGGL((symv_tile_kernel<T>), dim3(w.ntile_lower, w.q), dim3(256), 0, st, (const T*)(w.base + w.off_V),
                           w.mat, w.npad, (const T*)b, (double*)(w.base + w.off_part), w.ntile_lower);
        CHECK_LAUNCH("symv_tile_kernel");
        hipLaunchKernelGGL((symv_reduce_kernel<T, TS>), dim3(w.nb, w.q), dim3(256), 0, st,
                           (const double*)(w.base + w.off_part), w.ntile_lower, w.npad, w.nb, z);
    }
    CHECK_LAUNCH("symv_reduce_kernel");
    // (float32: the noise gradient comes from c = (C o s s^T) z after this launch, so no extra blocks here)
    for_kern(w.kern, [&](auto kern) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(w.ntile_lower + (sizeof(T) == 4 ? 0 : w.p), w.q), dim3(256), 0, st,
                               (const T*)(w.base + w.off_V), w.mat, w.n, w.npad, w.d, w.p, (const T*)x, (const T*)sr,
                               (const T*)(w.base + w.off_z), theta, (double*)(w.base + w.off_part), w.ntile_lower, (const T*)Y,
                               (const T*)(w.base + w.off_b), out, (double*)(w.base + w.off_cpart));
        };
        if (w.d > DMAX) go(grad_kernel_wide<T, decltype(kern)::value>);
        else for_dim(w.d, [&](auto dd) { go(grad_kernel<T, decltype(dd)::value, decltype(kern)::value>); });
    });
    CHECK_LAUNCH("grad_kernel");
    const double* cvec = nullptr;
    if constexpr (sizeof(T) == 4) {
        double* c = (double*)(w.base + w.off_c);
        hipLaunchKernelGGL(cvec_reduce_kernel, dim3(w.nb, w.q), dim3(256), 0, st, (const double*)(w.base + w.off_cpart),
                           w.ntile_lower, w.npad, w.nb, c);
        CHECK_LAUNCH("cvec_reduce_kernel");
        hipLaunchKernelGGL((gsig_c_kernel<T>), dim3(w.p, w.q), dim3(256), 0, st, w.n, w.npad, w.d, w.p, (const T*)Y,
                           (const double*)c, theta, out);
        CHECK_LAUNCH("gsig_c_kernel");
        cvec = c;
    }
    hipLaunchKernelGGL((finalize_kernel<T>), dim3(w.q), dim3(256), 0, st, w.n, w.npad, w.d, w.p, w.ntile_lower,
                       (const T*)Y, (const T*)b, (const T*)z, (const double*)(w.base + w.off_part),
                       (const double*)(w.base + w.off_logdet), (const int*)(w.base + w.off_info), theta, out, cvec);
    CHECK_LAUNCH("finalize_kernel");
    return 0;
}

// The rank's share of the reduced vector, assembled on the device (one workgroup, fixed summation order):
//   vec = [ sum_k (half_logdet_k - quad_k / (2 D_k)) | sum_k info_k | g_ell (q x d) | g_scale (q) | g_nug (q) | g_sigma (p) | guard ]
// component-local slots are written at the GLOBAL component index comp[i]; g_sigma_a = sum_k psi_k[a] gsig_k[a] / (2 D_k).
// guard: a word of the caller's (a hash of the parameter vector the rank evaluated) that travels through the all-reduce in
// the last slot, so that ranks which have drifted apart are detected at the first evaluation instead of diverging.
__global__ __launch_bounds__(256) void pack_partial_kernel(int d, int p, int q_local, int q_total,
                                                           const int* __restrict__ comp, const double* __restrict__ theta,
                                                           const double* __restrict__ out, const double* __restrict__ guard,
                                                           double* __restrict__ vec) {
    const int tid = threadIdx.x;
    const int tw = d + 3 + p, ow = d + 5 + p;
    const int off_s = 2 + q_total * d, off_n = off_s + q_total, off_g = off_n + q_total;
    for (int e = tid; e < off_g; e += 256) vec[e] = 0.0;
    __syncthreads();
    if (tid == 0) {
        vec[off_g + p] = guard ? guard[0] : 0.0;
        double v = 0.0, bad_sum = 0.0;
        for (int i = 0; i < q_local; ++i) {
            const double* o = out + (size_t)i * ow;
            v += o[0] - o[1] / (2.0 * theta[(size_t)i * tw + d + 2]);
            bad_sum += o[2];
        }
        vec[0] = v;
        vec[1] = bad_sum;
    }
    for (int e = tid; e < q_local * (d + 2); e += 256) {
        const int i = e / (d + 2), j = e - i * (d + 2);
        const int k = comp[i];
        const double val = out[(size_t)i * ow + 3 + j];
        if (j < d) vec[2 + k * d + j] = val;
        else if (j == d) vec[off_s + k] = val;
        else vec[off_n + k] = val;
    }
    for (int a = tid; a < p; a += 256) {
        double s = 0.0;
        for (int i = 0; i < q_local; ++i) {
            const double* th = theta + (size_t)i * tw;
            s += 0.5 * th[d + 3 + a] * out[(size_t)i * ow + 5 + d + a] / th[d + 2];
        }
        vec[off_g + a] = s;
    }
}

int check_common(int dtype, int n, int d, int p, int q, int kernel_id = 0) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (kernel_id != LCGP_KERNEL_MATERN32 && kernel_id != LCGP_KERNEL_SE && kernel_id != LCGP_KERNEL_MATERN52)
        return bad("kernel_id must be 0 (Matern-3/2), 1 (squared exponential) or 2 (Matern-5/2)");
    if (n < 1) return bad("n < 1");
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (p < 1) return bad("p < 1");
    if (q < 1 || q > 65535) return bad("q_local must be in [1, 65535]");
    return 0;
}

inline int resolve_sched(const lcgp_sched* in, lcgp_sched& out) {
    out = in ? *in : default_sched();
    return check_sched(out);
}

template <typename T>
int do_matern(hipStream_t st, int kern, int n1, int n2, int d, const void* x1, const void* x2, const ThetaArg& th, int same,
              void* out) {
    dim3 grid((n2 + TS - 1) / TS, (n1 + TS - 1) / TS);
    for_kern(kern, [&](auto k) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(k)::value>), grid, dim3(256), 0, st, (T*)out, n2, n1, n2, d, (const T*)x1,
                           (const T*)x2, th, (const double*)nullptr, same, (const T*)nullptr, n1, n2, 0, (size_t)0,
                           (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    return 0;
}

// rows of the padded cross-covariance block: whole 128-tiles when there are at least 128 new inputs (the MFMA products
// then run on the 128x128 8-wave tile kernel), whole 64-tiles otherwise
inline int predict_pad(int n0) { return n0 >= 128 ? round_up(n0, 2 * TS) : round_up(n0, TS); }

// C_k = A_k op B_k (an OP_PRED_* product of the tile kernel) for all local components: A and C are `rows` x ld slabs sA
// apart, B_k ld x ld matrices sB apart, ld = nb 64-tiles.  128x128 tiles when rows is a multiple of 128, 64x64 tiles otherwise.
template <typename T, int OP>
int launch_pred(hipStream_t st, const T* A, const T* B, T* C, size_t sA, size_t sB, int ld, int rows, int nb, int q,
                size_t sC = 0 /*0 = sA*/, bool small = false /*64x64 tiles whatever rows is*/, int ldc = 0 /*row length of C; 0 = ld*/) {
    GemmArgs g;
    g.A = A; g.B = B; g.C = C;
    g.sA = sA; g.sB = sB; g.sC = sC ? sC : sA; g.ldA = g.ldB = ld; g.ldC = ldc ? ldc : ld; g.p1 = g.p2 = g.p3 = 0;
    if (rows % (2 * TS) == 0 && !small) {
        g.nb = nb / 2; g.p0 = rows / (2 * TS);
        return launch_gemm<T, OP, 128>(st, g, g.p0 * g.nb, q);
    }
    g.nb = nb; g.p0 = rows / TS;
    return launch_gemm<T, OP, 64>(st, g, g.p0 * g.nb, q);
}

// X_k = c0k o sr^T (one launch; zero padded to n0pad rows) and U_k = X_k W_k^T (one launch of the tile kernel, k tiles only
// up to the diagonal: W is lower triangular) for all local components: q slabs n0pad x npad each
template <typename T>
int form_xu(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n0, int n0pad, const void* x0,
            int same, T* X, T* U) {
    const size_t slab = (size_t)n0pad * w.npad;
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(w.nb, n0pad / TS, w.q), dim3(256), 0, st, X, w.npad, n0,
                           w.n, w.d, (const T*)x0, (const T*)x, dummy, theta, same, (const T*)sr, n0pad, w.npad, w.d + 3 + w.p, slab,
                           (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    return launch_pred<T, OP_PRED_U>(st, X, (const T*)(w.base + w.off_W), U, slab, w.mat, w.npad, n0pad, w.nb, w.q);
}

// K6, all local components in every launch: X_k and U_k (form_xu), then the row reductions.
template <typename T>
int do_predict(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n0, const void* x0,
               int same, void* scratch, double* ghat, double* gvar, int ldo) {
    const int n0pad = predict_pad(n0);
    const size_t slab = (size_t)n0pad * w.npad;
    T* X = (T*)scratch;                 // q slabs n0pad x npad : c0k o sr^T (zero padded)
    T* U = X + slab * w.q;              // q slabs n0pad x npad : X W^T = (L^-1 X^T)^T
    int rc = form_xu<T>(st, w, x, sr, theta, n0, n0pad, x0, same, X, U);
    if (rc) return rc;
    hipLaunchKernelGGL((pred_reduce_kernel<T>), dim3(n0, w.q), dim3(64), 0, st, (const T*)X, (const T*)U, slab, slab, w.npad, w.n,
                       (const T*)(w.base + w.off_z), w.npad, theta, w.d + 3 + w.p, w.d, ldo, ghat, gvar);
    CHECK_LAUNCH("pred_reduce_kernel");
    return 0;
}

// K7 for all local components: do_predict with same = 0 (ghat / gvar bitwise those of lcgp_predict), then V_k = U_k W_k into
// the X slab (free once the row reductions have read it; one launch of the tile kernel, k tiles from the diagonal of W
// down), then the fused contraction (pgrad_kernel).  Scratch: that of lcgp_predict.
template <typename T>
int do_predict_grad(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n0, const void* x0,
                    void* scratch, double* ghat, double* gvar, double* dghat, double* dgvar, int ldo) {
    int rc = do_predict<T>(st, w, x, sr, theta, n0, x0, 0, scratch, ghat, gvar, ldo);
    if (rc) return rc;
    const int n0pad = predict_pad(n0);
    const size_t slab = (size_t)n0pad * w.npad;
    T* X = (T*)scratch;
    T* U = X + slab * w.q;
    rc = launch_pred<T, OP_PRED_V>(st, U, (const T*)(w.base + w.off_W), X, slab, w.mat, w.npad, n0pad, w.nb, w.q);
    if (rc) return rc;
    const int wide = w.d > 16;
    dim3 grid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, wide ? (w.d + DMAX - 1) / DMAX : 1);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((pgrad_kernel<T, decltype(dd)::value, decltype(kern)::value>), grid, dim3(256), 0, st, (const T*)x0,
                               n0, (const T*)x, (const T*)sr, w.n, w.d, theta, w.d + 3 + w.p, (const T*)(w.base + w.off_z), w.npad,
                               (const T*)X, slab, ldo, dghat, dgvar);
        });
    });
    CHECK_LAUNCH("pgrad_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Joint posterior covariance over new inputs and correlated draws (no counterpart in the reference, whose predict is
// marginal only).  The covariance lives in the matrix slot of a SECOND workspace carved for n = n0 (n0pad = round_up(n0,
// 128), the padding the factorisation expects), so lcgp_potrf_logdet factors it unchanged.
// ---------------------------------------------------------------------------------------------------
inline int cov_pad(int n0) { return round_up(n0, 2 * TS); }

// diagonal of Sigma_k + tau_k I (tau_k = jitter scale_k) and the identity block of the padding (rows n0 .. n0pad: zero from
// cross_kernel and from the zero rows of U, so only the diagonal needs a value)
template <typename T>
__global__ __launch_bounds__(256) void cov_diag_kernel(T* __restrict__ M, size_t mat, int n0, int n0pad,
                                                       const double* __restrict__ theta, int tw, int d, double jitter) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= n0pad) return;
    T* e = M + (size_t)k * mat + (size_t)i * n0pad + i;
    *e = i < n0 ? (T)((double)*e + jitter * theta[(size_t)k * tw + d]) : (T)1;
}

// zeroes the strict upper triangle of the 128x128 diagonal tiles of a factor: the draw product (OP_PRED_U) reads whole
// diagonal tiles and relies on stored zeros there, which the factorisation leaves only inside its 64x64 diagonal blocks
template <typename T>
__global__ __launch_bounds__(256) void diag_tile_upper_zero_kernel(T* __restrict__ M, size_t mat, int ld) {
    const int t = blockIdx.x, k = blockIdx.y;
    T* base = M + (size_t)k * mat + (size_t)t * 2 * TS * ld + (size_t)t * 2 * TS;
    for (int e = threadIdx.x; e < 4 * TS * TS; e += 256) {
        const int i = e / (2 * TS), j = e - i * (2 * TS);
        if (j > i) base[(size_t)i * ld + j] = (T)0;
    }
}

// dense eps (q, S, n0) -> zero-padded (q, Spad, n0pad)
template <typename T>
__global__ __launch_bounds__(256) void eps_pack_kernel(const T* __restrict__ eps, int S, int n0, T* __restrict__ E, int n0pad,
                                                       size_t slab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y, k = blockIdx.z;
    if (i >= n0pad) return;
    E[(size_t)k * slab + (size_t)s * n0pad + i] = (s < S && i < n0) ? eps[((size_t)k * S + s) * n0 + i] : (T)0;
}

// out[k, s, i] = ghat[k, i] + (L_k E_k)^T[s, i]
template <typename T>
__global__ __launch_bounds__(256) void draw_out_kernel(const T* __restrict__ G, int n0pad, size_t slab, int S, int n0,
                                                       const double* __restrict__ ghat, int ldg, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y, k = blockIdx.z;
    if (i >= n0) return;
    out[((size_t)k * S + s) * n0 + i] = ghat[(size_t)k * ldg + i] + (double)G[(size_t)k * slab + (size_t)s * n0pad + i];
}

// Sigma_k + tau_k I for all local components:  C00_k = kernel(x0, x0) with the nugget on the diagonal (cross_kernel, same =
// 1), X_k = c0k o sr^T and U_k = X_k W_k^T exactly as do_predict forms them (form_xu), then ONE launch of the tile kernel
// C00_k -= D_k U_k U_k^T over the lower tiles (K = npad), then the diagonal.
template <typename T>
int do_predict_cov(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n0, const void* x0,
                   int same, void* scratch, const Ws& cw, double jitter) {
    const int n0pad = cw.npad;
    const size_t slab = (size_t)n0pad * w.npad;
    T* X = (T*)scratch;
    T* U = X + slab * w.q;
    T* M = (T*)(cw.base + cw.off_M);
    const int tw = w.d + 3 + w.p;
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(n0pad / TS, n0pad / TS, w.q), dim3(256), 0, st, M, n0pad,
                           n0, n0, w.d, (const T*)x0, (const T*)x0, dummy, theta, 1, (const T*)nullptr, n0pad, n0pad, tw, cw.mat,
                           (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    int rc = form_xu<T>(st, w, x, sr, theta, n0, n0pad, x0, same, X, U);
    if (rc) return rc;
    GemmArgs h;
    h.A = U; h.B = U; h.C = M;
    h.sA = h.sB = slab; h.sC = cw.mat; h.ldA = h.ldB = w.npad; h.ldC = n0pad;
    h.p1 = tw; h.p2 = w.d + 2; h.p3 = 0;
    h.theta = theta;
    // 64x64 tiles: the 128-tile instances of this op do not compile clean -- fp64 needs 12 registers more than the 128 a
    // lane has at 4 waves per SIMD (a spill in the k loop; OP_PRED_U, the same loop, fits in 127), and in fp32 the compiler
    // moves registers of the hand-counted prefetch before their wait (tools/check_counted_prefetch.py)
    const int t64 = n0pad / TS;
    h.nb = t64; h.p0 = w.npad / TS;
    rc = launch_gemm<T, OP_PRED_COV, 64>(st, h, t64 * (t64 + 1) / 2, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL((cov_diag_kernel<T>), dim3((n0pad + 255) / 256, w.q), dim3(256), 0, st, M, cw.mat, n0, n0pad, theta, tw,
                       w.d, jitter);
    CHECK_LAUNCH("cov_diag_kernel");
    return 0;
}

// draws g_k = ghat_k + L_k eps_k for S draws per component, L_k the factor lcgp_potrf_logdet left in the cov workspace:
// (L_k E_k)^T = E_k^T L_k^T is the product OP_PRED_U forms (X W^T with W lower triangular), X = E_k^T padded to whole tiles
template <typename T>
int do_sample(hipStream_t st, const Ws& cw, int S, const void* eps, const double* ghat, int ldg, void* scratch, double* out) {
    const int n0pad = cw.npad, Spad = round_up(S, 2 * TS);
    const size_t slab = (size_t)Spad * n0pad;
    T* E = (T*)scratch;
    T* G = E + slab * cw.q;
    T* M = (T*)(cw.base + cw.off_M);
    hipLaunchKernelGGL((diag_tile_upper_zero_kernel<T>), dim3(n0pad / (2 * TS), cw.q), dim3(256), 0, st, M, cw.mat, n0pad);
    CHECK_LAUNCH("diag_tile_upper_zero_kernel");
    hipLaunchKernelGGL((eps_pack_kernel<T>), dim3((n0pad + 255) / 256, Spad, cw.q), dim3(256), 0, st, (const T*)eps, S, cw.n, E,
                       n0pad, slab);
    CHECK_LAUNCH("eps_pack_kernel");
    int rc = launch_pred<T, OP_PRED_U>(st, E, M, G, slab, cw.mat, n0pad, Spad, n0pad / TS, cw.q);
    if (rc) return rc;
    hipLaunchKernelGGL((draw_out_kernel<T>), dim3((cw.n + 255) / 256, S, cw.q), dim3(256), 0, st, (const T*)G, n0pad, slab, S,
                       cw.n, ghat, ldg, out);
    CHECK_LAUNCH("draw_out_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Conditioning on new runs without refactorising (no counterpart in the reference): lcgp_condition_prepare /
// lcgp_condition_predict (lcgp_hip.h).  The fitted workspace is only read.  Per local component, for m new unique inputs xn:
//     U_n = (c(xn, x) o sr^T) W^T,  S = C(xn, xn) - D U_n U_n^T + diag(1 / (D r_i)),  L_S L_S^T = S,  v = L_S^-1 (t - ghat(xn))
// and for new inputs x0:  Sigma_0n = C^x(x0, xn) - D U_0 U_n^T,  T = Sigma_0n L_S^-T,  ghat += T v,  gvar -= rowsum(T o T).
// S lives in the matrix slot of a SECOND workspace carved for n = m (as the joint covariance's); the state keeps U_n, a dense
// copy of L_S^-1 with its strict upper triangle zeroed (the product that forms T reads whole tiles) and v.
// ---------------------------------------------------------------------------------------------------
struct CondLay {
    int npad, mpad;
    size_t off_U, off_W, off_v, total;      // state: U_n (q mpad npad elements), L_S^-1 (q mpad^2 elements), v (q mpad doubles)
};

inline CondLay cond_carve(int dtype, int n, int q, int m) {
    CondLay L;
    const size_t esz = dtype == LCGP_F64 ? 8 : 4;
    L.npad = round_up(n, 2 * TS);
    L.mpad = cov_pad(m);
    size_t o = 0;
    L.off_U = o; o = align256(o + (size_t)q * L.mpad * L.npad * esz);
    L.off_W = o; o = align256(o + (size_t)q * L.mpad * L.mpad * esz);
    L.off_v = o; o = align256(o + (size_t)q * L.mpad * sizeof(double));
    L.total = o;
    return L;
}

// scratch of the preparation: X of the conditioning inputs (q mpad npad elements), then ghat / gvar there (2 q mpad doubles)
inline size_t cond_prepare_scratch(int dtype, int n, int q, int m) {
    const size_t esz = dtype == LCGP_F64 ? 8 : 4;
    const size_t mpad = cov_pad(m), npad = round_up(n, 2 * TS);
    return align256((size_t)q * mpad * npad * esz) + align256(2 * (size_t)q * mpad * sizeof(double));
}

// scratch of a prediction pass: X and U of the new inputs (2 q n0pad npad elements), Sigma_0n and T (2 q n0pad mpad elements)
inline size_t cond_predict_scratch(int dtype, int n, int q, int m, int n0) {
    const size_t esz = dtype == LCGP_F64 ? 8 : 4;
    const size_t mpad = cov_pad(m), npad = round_up(n, 2 * TS), n0pad = predict_pad(n0);
    return align256(2 * (size_t)q * n0pad * npad * esz) + align256(2 * (size_t)q * n0pad * mpad * esz);
}

// diagonal of S = Sigma_nn + diag(tau), tau_i = 1 / (D_k r_i) (r = NULL: ones), and the identity of the padding
template <typename T>
__global__ __launch_bounds__(256) void cond_diag_kernel(T* __restrict__ M, size_t mat, int m, int mpad,
                                                        const double* __restrict__ theta, int tw, int d,
                                                        const double* __restrict__ r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= mpad) return;
    T* e = M + (size_t)k * mat + (size_t)i * mpad + i;
    const double D = theta[(size_t)k * tw + d + 2];
    *e = i < m ? (T)((double)*e + 1.0 / (D * (r ? r[i] : 1.0))) : (T)1;
}

// dense copy of the lower triangle of L_S^-1 (W slot of the cond workspace) into the state, zeros above the diagonal
template <typename T>
__global__ __launch_bounds__(256) void cond_copy_kernel(const T* __restrict__ W, size_t mat, int mpad, T* __restrict__ dst) {
    const int i = blockIdx.x, j = blockIdx.y * blockDim.x + threadIdx.x, k = blockIdx.z;     // (rows on grid.x: no 65535 limit)
    if (j >= mpad) return;
    const size_t at = (size_t)k * mat + (size_t)i * mpad + j;
    dst[at] = j <= i ? W[at] : (T)0;
}

// v[k, i] = sum_{j <= i} L_S^-1[i, j] (t[k, j] - ghat_n[k, j])    (one wave per row i; zero on the padding)
template <typename T>
__global__ __launch_bounds__(64) void cond_v_kernel(const T* __restrict__ Wi, size_t mat, int m, int mpad,
                                                    const double* __restrict__ t, const double* __restrict__ gh, int ldg,
                                                    double* __restrict__ v) {
    const int i = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    double s = 0.0;
    if (i < m) {
        const T* row = Wi + (size_t)k * mat + (size_t)i * mpad;
        for (int j = lane; j <= i; j += 64) s += (double)row[j] * (t[(size_t)k * m + j] - gh[(size_t)k * ldg + j]);
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    }
    if (lane == 0) v[(size_t)k * mpad + i] = s;
}

// ghat[k, r] += sum_j T[r, j] v[k, j] ;  gvar[k, r] -= sum_j T[r, j]^2        (one wave per row, pred_reduce_kernel's order)
template <typename T>
__global__ __launch_bounds__(64) void cond_reduce_kernel(const T* __restrict__ Tm, size_t slab, int ld, int m,
                                                         const double* __restrict__ v, int mpad, int ldo,
                                                         double* __restrict__ ghat, double* __restrict__ gvar) {
    const int r = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const T* Tr = Tm + (size_t)k * slab + (size_t)r * ld;
    const double* vk = v + (size_t)k * mpad;
    double s1 = 0.0, s2 = 0.0;
    for (int j = lane; j < m; j += 64) {
        const double u = (double)Tr[j];
        s1 += u * vk[j];
        s2 += u * u;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
    if (lane == 0) { ghat[(size_t)k * ldo + r] += s1; gvar[(size_t)k * ldo + r] -= s2; }
}

template <typename T>
int do_condition_prepare(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int m, const void* xn,
                         const double* t, const double* r, void* scratch, const Ws& cw, void* state, int* info) {
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const CondLay L = cond_carve(dtype, w.n, w.q, m);
    const int mpad = L.mpad, tw = w.d + 3 + w.p;
    const size_t slab = (size_t)mpad * w.npad;
    T* X = (T*)scratch;
    double* gh = (double*)((char*)scratch + align256((size_t)w.q * slab * sizeof(T)));
    double* gv = gh + (size_t)w.q * mpad;
    T* Un = (T*)((char*)state + L.off_U);
    T* Wi = (T*)((char*)state + L.off_W);
    double* v = (double*)((char*)state + L.off_v);
    T* M = (T*)(cw.base + cw.off_M);
    // U_n and ghat(xn): the launches of lcgp_predict with same = 0 (a conditioning input is a new input)
    int rc = form_xu<T>(st, w, x, sr, theta, m, mpad, xn, 0, X, Un);
    if (rc) return rc;
    hipLaunchKernelGGL((pred_reduce_kernel<T>), dim3(m, w.q), dim3(64), 0, st, (const T*)X, (const T*)Un, slab, slab, w.npad, w.n,
                       (const T*)(w.base + w.off_z), w.npad, theta, tw, w.d, mpad, gh, gv);
    CHECK_LAUNCH("pred_reduce_kernel");
    // S: C(xn, xn) with the nugget on the diagonal, minus D U_n U_n^T over the lower tiles (the launch of lcgp_predict_cov),
    // plus tau_i on the diagonal
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(mpad / TS, mpad / TS, w.q), dim3(256), 0, st, M, mpad, m,
                           m, w.d, (const T*)xn, (const T*)xn, dummy, theta, 1, (const T*)nullptr, mpad, mpad, tw, cw.mat,
                           (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    GemmArgs h;
    h.A = Un; h.B = Un; h.C = M;
    h.sA = h.sB = slab; h.sC = cw.mat; h.ldA = h.ldB = w.npad; h.ldC = mpad;
    h.p1 = tw; h.p2 = w.d + 2; h.p3 = 0;
    h.theta = theta;
    const int t64 = mpad / TS;
    h.nb = t64; h.p0 = w.npad / TS;
    rc = launch_gemm<T, OP_PRED_COV, 64>(st, h, t64 * (t64 + 1) / 2, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL((cond_diag_kernel<T>), dim3((mpad + 255) / 256, w.q), dim3(256), 0, st, M, cw.mat, m, mpad, theta, tw, w.d, r);
    CHECK_LAUNCH("cond_diag_kernel");
    // L_S and L_S^-1 by the unchanged factorisation and triangular inverse on the second workspace
    const lcgp_sched sc = default_sched();
    rc = do_potrf<T>(st, cw, sc);
    if (rc) return rc;
    rc = do_trtri<T>(st, cw, sc);
    if (rc) return rc;
    hipLaunchKernelGGL(copy_stats_kernel, dim3((w.q + 63) / 64), dim3(64), 0, st, (const double*)(cw.base + cw.off_logdet),
                       (const int*)(cw.base + cw.off_info), (double*)nullptr, info, w.q);
    CHECK_LAUNCH("copy_stats");
    hipLaunchKernelGGL((cond_copy_kernel<T>), dim3(mpad, (mpad + 255) / 256, w.q), dim3(256), 0, st,
                       (const T*)(cw.base + cw.off_W), cw.mat, mpad, Wi);
    CHECK_LAUNCH("cond_copy_kernel");
    hipLaunchKernelGGL((cond_v_kernel<T>), dim3(mpad, w.q), dim3(64), 0, st, (const T*)Wi, (size_t)mpad * mpad, m, mpad, t,
                       (const double*)gh, mpad, v);
    CHECK_LAUNCH("cond_v_kernel");
    return 0;
}

template <typename T>
int do_condition_predict(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const void* state, int m,
                         const void* xn, int n0, const void* x0, void* scratch, double* ghat, double* gvar, int ldo) {
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const CondLay L = cond_carve(dtype, w.n, w.q, m);
    const int mpad = L.mpad, tw = w.d + 3 + w.p, n0pad = predict_pad(n0);
    const size_t slab = (size_t)n0pad * w.npad, cslab = (size_t)n0pad * mpad;
    const T* Un = (const T*)((const char*)state + L.off_U);
    const T* Wi = (const T*)((const char*)state + L.off_W);
    const double* v = (const double*)((const char*)state + L.off_v);
    T* U0 = (T*)scratch + slab * w.q;
    T* Sg = (T*)((char*)scratch + align256(2 * (size_t)w.q * slab * sizeof(T)));
    T* Tm = Sg + cslab * w.q;
    // U_0, ghat, gvar exactly as lcgp_predict(same = 0)
    int rc = do_predict<T>(st, w, x, sr, theta, n0, x0, 0, scratch, ghat, gvar, ldo);
    if (rc) return rc;
    // Sigma_0n = C^x(x0, xn) - D U_0 U_n^T on all tiles (zero on the padding rows and columns)
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(mpad / TS, n0pad / TS, w.q), dim3(256), 0, st, Sg, mpad, n0,
                           m, w.d, (const T*)x0, (const T*)xn, dummy, theta, 0, (const T*)nullptr, n0pad, mpad, tw, cslab,
                           (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    GemmArgs h;
    h.A = U0; h.B = Un; h.C = Sg;
    h.sA = slab; h.sB = (size_t)mpad * w.npad; h.sC = cslab; h.ldA = h.ldB = w.npad; h.ldC = mpad;
    h.nb = 0; h.p0 = w.npad / TS; h.p1 = mpad / TS; h.p2 = tw; h.p3 = w.d + 2;
    h.theta = theta;
    // (64x64 tiles, the instance OP_PRED_COV runs on; a 128x128 instance of this op has not been compiled or measured)
    rc = launch_gemm<T, OP_COND_CROSS, 64>(st, h, (n0pad / TS) * (mpad / TS), w.q);
    if (rc) return rc;
    // T = Sigma_0n L_S^-T: the product of lcgp_predict's U with X := Sigma_0n, W := L_S^-1
    rc = launch_pred<T, OP_PRED_U>(st, Sg, Wi, Tm, cslab, (size_t)mpad * mpad, mpad, n0pad, mpad / TS, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL((cond_reduce_kernel<T>), dim3(n0, w.q), dim3(64), 0, st, (const T*)Tm, cslab, mpad, m, v, mpad, ldo, ghat,
                       gvar);
    CHECK_LAUNCH("cond_reduce_kernel");
    return 0;
}

// Box-averaged predictions of the fitted model (state = NULL, m = 0) or of a conditioned view, all local components in every
// launch (lcgp_predict_marginal, lcgp_condition_predict_marginal).  Fitted model: the table of 1-D averages (marg_table_kernel),
// the rows (cross_kernel with the masks), U = X W^T (the launch of form_xu) and the row reductions with the per-row prior.
// View: averaging commutes with conditioning, so the pass is do_condition_predict's with both row kernels replaced by their
// masked instances -- a second table over the view's inputs xn (marg_table_kernel with x := xn, n := m, npad := mpad), the
// masked rows against xn (no sr, no nugget) into Sigma_0n, then OP_COND_CROSS, T and cond_reduce_kernel as there.
// The reference row (MargRef) adds launches BEHIND those and changes none of them: ref_out copies the widened row [U_r | T_r] of
// pass row ref_row out, ref_in gives gcov = the covariance of every row's average with that of the row ref_in belongs to.
// Scratch: X and U as in do_predict, then the table (q d npad doubles) and I2 (q d doubles); on a view that of
// do_condition_predict, then the table and I2, then the table over xn (q d mpad doubles).
struct MargRef {
    int row = 0;                                  // pass row written to out
    void* out = nullptr;                          // q (npad + mpad) elements, or NULL
    const void* in = nullptr;                     // the widened row of the reference row, or NULL
    const void* x = nullptr;                      // its d values (entries under its mask are never read)
    const unsigned char* mask = nullptr;          // its d mask bytes
    double* gcov = nullptr;                       // q rows of ldo
};

template <typename T>
int do_predict_marginal(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const void* state, int m,
                        const void* xn, int n0, const void* x0, const unsigned char* mask, const double* box, void* scratch,
                        double* ghat, double* gvar, int ldo, const MargRef& ref) {
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const int n0pad = predict_pad(n0);
    const size_t slab = (size_t)n0pad * w.npad;
    const int tw = w.d + 3 + w.p;
    const int mpad = state ? cov_pad(m) : 0;
    const size_t cslab = (size_t)n0pad * mpad;
    T* X = (T*)scratch;
    T* U = X + slab * w.q;
    T* Sg = state ? (T*)((char*)scratch + align256(2 * (size_t)w.q * slab * sizeof(T))) : nullptr;
    T* Tm = state ? Sg + cslab * w.q : nullptr;
    double* tab = state ? (double*)((char*)scratch + cond_predict_scratch(dtype, w.n, w.q, m, n0)) : (double*)(U + slab * w.q);
    double* i2 = tab + (size_t)w.q * w.d * w.npad;
    double* tabn = i2 + (size_t)w.q * w.d;
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((marg_table_kernel<T, decltype(kern)::value>), dim3((w.npad + 255) / 256, w.d, w.q), dim3(256), 0, st,
                           (const T*)x, w.n, w.npad, w.d, theta, tw, box, tab, i2);
    });
    CHECK_LAUNCH("marg_table_kernel");
    if (state) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((marg_table_kernel<T, decltype(kern)::value>), dim3((mpad + 255) / 256, w.d, w.q), dim3(256), 0, st,
                               (const T*)xn, m, mpad, w.d, theta, tw, box, tabn, i2);      // (I2 again: the same values)
        });
        CHECK_LAUNCH("marg_table_kernel (view inputs)");
    }
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value, const unsigned char*, const double*>), dim3(w.nb, n0pad / TS, w.q),
                           dim3(256), 0, st, X, w.npad, n0, w.n, w.d, (const T*)x0, (const T*)x, dummy, theta, 0, (const T*)sr, n0pad,
                           w.npad, tw, slab, (const int*)nullptr, mask, (const double*)tab);
    });
    CHECK_LAUNCH("cross_kernel (marginal rows)");
    int rc = launch_pred<T, OP_PRED_U>(st, X, (const T*)(w.base + w.off_W), U, slab, w.mat, w.npad, n0pad, w.nb, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL((marg_reduce_kernel<T>), dim3(n0, w.q), dim3(64), 0, st, (const T*)X, (const T*)U, slab, w.npad, w.n,
                       (const T*)(w.base + w.off_z), w.npad, theta, tw, w.d, mask, (const double*)i2, ldo, ghat, gvar);
    CHECK_LAUNCH("marg_reduce_kernel");
    if (state) {
        const CondLay L = cond_carve(dtype, w.n, w.q, m);
        const T* Un = (const T*)((const char*)state + L.off_U);
        const T* Wi = (const T*)((const char*)state + L.off_W);
        const double* v = (const double*)((const char*)state + L.off_v);
        // Sigma_0n = Cbar^x(x0, xn) - D U_0 U_n^T: the masked rows against the view's inputs (table rows mpad long, m columns)
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value, const unsigned char*, const double*>),
                               dim3(mpad / TS, n0pad / TS, w.q), dim3(256), 0, st, Sg, mpad, n0, m, w.d, (const T*)x0, (const T*)xn,
                               dummy, theta, 0, (const T*)nullptr, n0pad, mpad, tw, cslab, (const int*)nullptr, mask,
                               (const double*)tabn);
        });
        CHECK_LAUNCH("cross_kernel (marginal rows, view inputs)");
        GemmArgs h;
        h.A = U; h.B = Un; h.C = Sg;
        h.sA = slab; h.sB = (size_t)mpad * w.npad; h.sC = cslab; h.ldA = h.ldB = w.npad; h.ldC = mpad;
        h.nb = 0; h.p0 = w.npad / TS; h.p1 = mpad / TS; h.p2 = tw; h.p3 = w.d + 2;
        h.theta = theta;
        rc = launch_gemm<T, OP_COND_CROSS, 64>(st, h, (n0pad / TS) * (mpad / TS), w.q);
        if (rc) return rc;
        rc = launch_pred<T, OP_PRED_U>(st, Sg, Wi, Tm, cslab, (size_t)mpad * mpad, mpad, n0pad, mpad / TS, w.q);
        if (rc) return rc;
        hipLaunchKernelGGL((cond_reduce_kernel<T>), dim3(n0, w.q), dim3(64), 0, st, (const T*)Tm, cslab, mpad, m, v, mpad, ldo, ghat,
                           gvar);
        CHECK_LAUNCH("cond_reduce_kernel");
    }
    if (ref.out) {
        hipLaunchKernelGGL((marg_refrow_kernel<T>), dim3((w.npad + mpad + 255) / 256, w.q), dim3(256), 0, st, (const T*)U, slab, w.npad,
                           (const T*)Tm, cslab, mpad, ref.row, (T*)ref.out);
        CHECK_LAUNCH("marg_refrow_kernel");
    }
    if (ref.in) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((marg_refcov_kernel<T, decltype(kern)::value>), dim3(n0, w.q), dim3(64), 0, st, (const T*)U, slab,
                               w.npad, w.n, (const T*)Tm, cslab, mpad, state ? m : 0, (const T*)ref.in, theta, tw, w.d,
                               (const T*)x0, mask, (const T*)ref.x, ref.mask, box, (const double*)i2, ldo, ref.gcov);
        });
        CHECK_LAUNCH("marg_refcov_kernel");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Input gradients on a conditioned view (lcgp_condition_grad_prepare / lcgp_condition_predict_grad, lcgp_hip.h).  With
// w = L_S^-T v and z' = z - D W^T (U_n^T w) (once per view, the grad state) the view's mean is X_0 z' + C^x(x0, xn) w; with
// R = T L_S^-1, U' = U_0 - R U_n and V' = U' W (per pass) its variance has the gradient -2 D sum_j dc sr_j V' - 2 sum_a dc^x R:
// pgrad_kernel's contraction over n + m columns (pgrad_cond_kernel).
// ---------------------------------------------------------------------------------------------------
struct CondGradLay {
    size_t off_w, off_z, off_a, total;      // w (q mpad doubles), z' (q npad doubles), a = U_n^T w (q npad doubles; work area)
};

inline CondGradLay cond_grad_carve(int n, int q, int m) {
    CondGradLay L;
    const size_t mpad = cov_pad(m), npad = round_up(n, 2 * TS);
    size_t o = 0;
    L.off_w = o; o = align256(o + (size_t)q * mpad * sizeof(double));
    L.off_z = o; o = align256(o + (size_t)q * npad * sizeof(double));
    L.off_a = o; o = align256(o + (size_t)q * npad * sizeof(double));
    L.total = o;
    return L;
}

// out[k, c] = (zs ? zs[k, c] - D_k sum : sum),  sum = sum_{i < nrows, tri: i >= c} M_k[i, c] vec[k, i]   for c < ncols: the
// product with the TRANSPOSE of a row-major matrix, read along its rows (64 adjacent columns per wave, coalesced).  The four
// waves of a workgroup take the rows i = wave (mod 4) in ascending order, in double; their sums are added in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void cond_tmatvec_kernel(const T* __restrict__ M, size_t mat, int ld, int nrows, int ncols,
                                                           int tri, const double* __restrict__ vec, int ldv,
                                                           const T* __restrict__ zs, const double* __restrict__ theta, int tw,
                                                           int d, double* __restrict__ out, int ldo) {
    __shared__ double part[4][64];
    const int k = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const T* Mk = M + (size_t)k * mat;
    const double* vk = vec + (size_t)k * ldv;
    double s = 0.0;
    if (c < ncols) {
        int i = tri ? (blockIdx.x * 64) / 4 * 4 + wave : wave;         // (rows above the block's first column hold nothing)
        for (; i < nrows; i += 4)
            if (!tri || i >= c) s = fma((double)Mk[(size_t)i * ld + c], vk[i], s);
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < ncols) {
        const double t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        out[(size_t)k * ldo + c] = zs ? (double)zs[(size_t)k * ldo + c] - theta[(size_t)k * tw + d + 2] * t : t;
    }
}

// w (q x m) and z' (q x n) of the grad state without their padding (lcgp_condition_grad_fetch)
__global__ __launch_bounds__(256) void cond_grad_fetch_kernel(const double* __restrict__ wv, int mpad, int m,
                                                              const double* __restrict__ zd, int npad, int n,
                                                              double* __restrict__ w, double* __restrict__ z) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) w[(size_t)k * m + i] = wv[(size_t)k * mpad + i];
    if (i < n) z[(size_t)k * n + i] = zd[(size_t)k * npad + i];
}

template <typename T>
int do_condition_grad_prepare(hipStream_t st, const Ws& w, const double* theta, const void* state, int m, void* gstate) {
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const CondLay L = cond_carve(dtype, w.n, w.q, m);
    const CondGradLay G = cond_grad_carve(w.n, w.q, m);
    const int mpad = L.mpad, tw = w.d + 3 + w.p;
    const T* Un = (const T*)((const char*)state + L.off_U);
    const T* Wi = (const T*)((const char*)state + L.off_W);
    const double* v = (const double*)((const char*)state + L.off_v);
    double* wv = (double*)((char*)gstate + G.off_w);
    double* zd = (double*)((char*)gstate + G.off_z);
    double* a = (double*)((char*)gstate + G.off_a);
    // w = L_S^-T v (zero on the padding: no row below m is read)
    hipLaunchKernelGGL((cond_tmatvec_kernel<T>), dim3(mpad / 64, w.q), dim3(256), 0, st, Wi, (size_t)mpad * mpad, mpad, m, mpad, 1,
                       v, mpad, (const T*)nullptr, theta, tw, w.d, wv, mpad);
    CHECK_LAUNCH("cond_tmatvec_kernel (w)");
    // a = U_n^T w
    hipLaunchKernelGGL((cond_tmatvec_kernel<T>), dim3(w.npad / 64, w.q), dim3(256), 0, st, Un, (size_t)mpad * w.npad, w.npad, m,
                       w.npad, 0, (const double*)wv, mpad, (const T*)nullptr, theta, tw, w.d, a, w.npad);
    CHECK_LAUNCH("cond_tmatvec_kernel (a)");
    // z' = z - D W^T a (W = L^-1 of the fitted workspace, lower triangular: the rows from the column down, below n)
    hipLaunchKernelGGL((cond_tmatvec_kernel<T>), dim3(w.npad / 64, w.q), dim3(256), 0, st, (const T*)(w.base + w.off_W), w.mat,
                       w.npad, w.n, w.npad, 1, (const double*)a, w.npad, (const T*)(w.base + w.off_z), theta, tw, w.d, zd, w.npad);
    CHECK_LAUNCH("cond_tmatvec_kernel (z')");
    return 0;
}

// One pass: the launches of lcgp_condition_predict (ghat' / gvar' bitwise its; they leave U_0 in the U slab and T behind
// Sigma_0n), R = T L_S^-1 over Sigma_0n (OP_PRED_V on the state's dense L_S^-1), U' = U_0 - R U_n in place (OP_COND_U), V' = U' W
// into the X slab (OP_PRED_V, as lcgp_predict_grad's V but on 64-row tiles) and the contraction over the n + m columns.
// Scratch: that of lcgp_condition_predict.
template <typename T>
int do_condition_predict_grad(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const void* state,
                              int m, const void* xn, const void* gstate, int n0, const void* x0, void* scratch, double* ghat,
                              double* gvar, double* dghat, double* dgvar, int ldo) {
    int rc = do_condition_predict<T>(st, w, x, sr, theta, state, m, xn, n0, x0, scratch, ghat, gvar, ldo);
    if (rc) return rc;
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const CondLay L = cond_carve(dtype, w.n, w.q, m);
    const CondGradLay G = cond_grad_carve(w.n, w.q, m);
    const int mpad = L.mpad, n0pad = predict_pad(n0);
    const size_t slab = (size_t)n0pad * w.npad, cslab = (size_t)n0pad * mpad;
    const T* Un = (const T*)((const char*)state + L.off_U);
    const T* Wi = (const T*)((const char*)state + L.off_W);
    T* X = (T*)scratch;
    T* U0 = X + slab * w.q;
    T* Rm = (T*)((char*)scratch + align256(2 * (size_t)w.q * slab * sizeof(T)));      // (Sigma_0n has been consumed)
    T* Tm = Rm + cslab * w.q;
    // 64x64 tiles for R and V' whatever the number of rows (as lcgp_variance_reduction_grad's G, Q and V): OP_PRED_V sums in a
    // different order on 128-row tiles, and a caller's split of the rows must not show in the Jacobians
    rc = launch_pred<T, OP_PRED_V>(st, Tm, Wi, Rm, cslab, (size_t)mpad * mpad, mpad, n0pad, mpad / TS, w.q, 0, true);
    if (rc) return rc;
    GemmArgs g;
    g.A = Rm; g.B = Un; g.C = U0;
    g.sA = cslab; g.sB = (size_t)mpad * w.npad; g.sC = slab; g.ldA = mpad; g.ldB = g.ldC = w.npad;
    g.p2 = g.p3 = 0;
    // 64x64 tiles, as OP_PRED_COV and OP_COND_CROSS: the 128-row instances of this op do not compile clean -- fp64 needs 15
    // registers more than the 128 a lane has at 4 waves per SIMD (spills), and in fp32 (106 registers) the compiler moves
    // registers of the hand-counted prefetch before their wait (tools/check_counted_prefetch.py)
    g.nb = w.nb; g.p0 = n0pad / TS; g.p1 = mpad / TS;
    rc = launch_gemm<T, OP_COND_U, 64>(st, g, g.p0 * g.nb, w.q);
    if (rc) return rc;
    rc = launch_pred<T, OP_PRED_V>(st, U0, (const T*)(w.base + w.off_W), X, slab, w.mat, w.npad, n0pad, w.nb, w.q, 0, true);
    if (rc) return rc;
    PgradCond<T> cs;
    cs.zd = (const double*)((const char*)gstate + G.off_z);
    cs.xn = (const T*)xn; cs.m = m;
    cs.wv = (const double*)((const char*)gstate + G.off_w); cs.mpad = mpad;
    cs.R = Rm; cs.rslab = cslab;
    const int wide = w.d > 16;
    dim3 grid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, wide ? (w.d + DMAX - 1) / DMAX : 1);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((pgrad_cond_kernel<T, decltype(dd)::value, decltype(kern)::value>), grid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, w.n, w.d, theta, w.d + 3 + w.p, w.npad, (const T*)X, slab,
                               ldo, dghat, dgvar, cs);
        });
    });
    CHECK_LAUNCH("pgrad_cond_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Closed-form cross-validation at fixed parameters (no counterpart in the reference).  With a = A_k^-1 (V slot), b_k, z_k
// and s = sr of the last lcgp_nll_grad, the model conditioned on all inputs but a set B predicts at x_B
//     ghat_B = S_B^-1 (b_B - M^-1 z_B) / D_k,   Sigma_B = S_B^-1 (M^-1 - I) S_B^-1 / D_k,   M = a[B, B]
// (lcgp_hip.h).  Leave-one-out is the case |B| = 1.  The fold matrices M live in the matrix slots of a second workspace
// carved for n = mmax (the largest fold) and q_local * F components, slot f * q_local + k; the unchanged lcgp_potrf_logdet
// and lcgp_potri turn them into M^-1 in its V slot.  Folds: `folds` = [fold_ptr (F + 1) | fold_idx (n)] device ints.
// ---------------------------------------------------------------------------------------------------

// leave-one-out for every training input i and local component k: one thread per (i, k), double arithmetic
template <typename T>
__global__ __launch_bounds__(256) void loo_kernel(const T* __restrict__ V, size_t mat, int n, int npad, const T* __restrict__ b,
                                                  const T* __restrict__ z, const T* __restrict__ sr,
                                                  const double* __restrict__ theta, int tw, int d, int ldo,
                                                  double* __restrict__ ghat, double* __restrict__ gvar) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= n) return;
    const double a = (double)V[(size_t)k * mat + (size_t)i * npad + i];
    const double bi = (double)b[(size_t)k * npad + i], zi = (double)z[(size_t)k * npad + i];
    const double s = sr ? (double)sr[i] : 1.0;
    const double Dk = theta[(size_t)k * tw + d + 2];
    const double ia = 1.0 / a;
    ghat[(size_t)k * ldo + i] = (bi - zi * ia) / (Dk * s);
    gvar[(size_t)k * ldo + i] = (ia - 1.0) / (Dk * s * s);
}

// slot s = f * q_local + k of the fold workspace <- a_k[B_f, B_f] in the form lcgp_kernel_build leaves for the factorisation:
// one workgroup per lower 64x64 tile (written whole; the strict upper tiles are never read), identity beyond m_f (the fold's
// own padding and that up to mpad).  a_k is read from its lower storage at (max, min).
template <typename T>
__global__ __launch_bounds__(256) void cv_gather_kernel(const T* __restrict__ V, size_t mat, int npad, const int* __restrict__ folds,
                                                        int F, int q_local, T* __restrict__ M, size_t cmat, int mpad) {
    const int s = blockIdx.y, f = s / q_local, k = s - f * q_local;
    int r, c;
    tri_decode(blockIdx.x, r, c);
    const int lo = folds[f], m = folds[f + 1] - lo;
    const int* __restrict__ idx = folds + F + 1 + lo;
    __shared__ int ri[TS], ci[TS];
    const int tid = threadIdx.x;
    if (tid < TS) {
        const int i = r * TS + tid;
        ri[tid] = i < m ? idx[i] : -1;
    } else if (tid < 2 * TS) {
        const int j = c * TS + tid - TS;
        ci[tid - TS] = j < m ? idx[j] : -1;
    }
    __syncthreads();
    const T* __restrict__ A = V + (size_t)k * mat;
    T* __restrict__ out = M + (size_t)s * cmat + (size_t)r * TS * mpad + (size_t)c * TS;
    for (int e = tid; e < TS * TS; e += 256) {
        const int ii = e / TS, jj = e - ii * TS;
        const int gi = ri[ii], gj = ci[jj];
        T v;
        if (gi >= 0 && gj >= 0) v = A[(size_t)max(gi, gj) * npad + min(gi, gj)];
        else v = (r == c && ii == jj) ? (T)1 : (T)0;
        out[(size_t)ii * mpad + jj] = v;
    }
}

// slot s = f * q_local + k: t = M^-1 z_B from the lower storage of M^-1 (V slot of the fold workspace), then ghat / gvar of the
// fold's inputs scattered to their positions fold_idx.  One workgroup per 64-row strip of M^-1: the 64x64 tiles of the strip
// pass through LDS (a tile above the diagonal is read as the transpose of its lower mirror), thread (row, g) sums the columns
// g, g + 4, .. of each tile in order and the four partials are added in a fixed order: no atomics, bitwise reproducible.
template <typename T>
__global__ __launch_bounds__(256) void cv_apply_kernel(const T* __restrict__ Mi, size_t cmat, int mpad, const int* __restrict__ folds,
                                                       int F, int q_local, const T* __restrict__ b, const T* __restrict__ z, int npad,
                                                       const T* __restrict__ sr, const double* __restrict__ theta, int tw, int d,
                                                       int ldo, double* __restrict__ ghat, double* __restrict__ gvar) {
    const int s = blockIdx.y, f = s / q_local, k = s - f * q_local, I = blockIdx.x;
    const int lo = folds[f], m = folds[f + 1] - lo;
    if (I * TS >= m) return;                     // (uniform per workgroup)
    const int* __restrict__ idx = folds + F + 1 + lo;
    const T* __restrict__ Ms = Mi + (size_t)s * cmat;
    const T* __restrict__ zk = z + (size_t)k * npad;
    __shared__ double tile[TS][TS + 1];
    __shared__ double zs[TS];
    __shared__ double part[4][TS];
    const int tid = threadIdx.x, row = tid & (TS - 1), g = tid >> 6;
    const int nJ = (m + TS - 1) / TS;
    double acc = 0.0;
    for (int J = 0; J < nJ; ++J) {
        const int tr = max(I, J), tc = min(I, J);        // the stored (lower) tile
        const T* __restrict__ src = Ms + (size_t)tr * TS * mpad + (size_t)tc * TS;
        for (int e = tid; e < TS * TS; e += 256) {
            const int a = e / TS, bb = e - a * TS;
            tile[a][bb] = (double)src[(size_t)a * mpad + bb];
        }
        if (tid < TS) {
            const int j = J * TS + tid;
            zs[tid] = j < m ? (double)zk[idx[j]] : 0.0;
        }
        __syncthreads();
        const int jend = min(TS, m - J * TS);
        for (int jj = g; jj < jend; jj += 4) {
            double v;
            if (J < I) v = tile[row][jj];
            else if (J > I) v = tile[jj][row];
            else v = row >= jj ? tile[row][jj] : tile[jj][row];
            acc += v * zs[jj];
        }
        __syncthreads();
    }
    part[g][row] = acc;
    __syncthreads();
    const int i = I * TS + tid;
    if (tid < TS && i < m) {
        const double t = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        const int gi = idx[i];
        const double mii = (double)Ms[(size_t)i * mpad + i];
        const double sv = sr ? (double)sr[gi] : 1.0;
        const double Dk = theta[(size_t)k * tw + d + 2];
        ghat[(size_t)k * ldo + gi] = ((double)b[(size_t)k * npad + gi] - t) / (Dk * sv);
        gvar[(size_t)k * ldo + gi] = (mii - 1.0) / (Dk * sv * sv);
    }
}

template <typename T>
int do_loo(hipStream_t st, const Ws& w, const void* sr, const double* theta, double* ghat, double* gvar, int ldo) {
    hipLaunchKernelGGL((loo_kernel<T>), dim3((w.n + 255) / 256, w.q), dim3(256), 0, st, (const T*)(w.base + w.off_V), w.mat, w.n,
                       w.npad, (const T*)(w.base + w.off_b), (const T*)(w.base + w.off_z), (const T*)sr, theta, w.d + 3 + w.p,
                       w.d, ldo, ghat, gvar);
    CHECK_LAUNCH("loo_kernel");
    return 0;
}

template <typename T>
int do_cv_gather(hipStream_t st, const Ws& w, const int* folds, int F, const Ws& cw) {
    const int nbm = cw.npad / TS;
    hipLaunchKernelGGL((cv_gather_kernel<T>), dim3(nbm * (nbm + 1) / 2, cw.q), dim3(256), 0, st, (const T*)(w.base + w.off_V),
                       w.mat, w.npad, folds, F, w.q, (T*)(cw.base + cw.off_M), cw.mat, cw.npad);
    CHECK_LAUNCH("cv_gather_kernel");
    return 0;
}

template <typename T>
int do_cv_apply(hipStream_t st, const Ws& w, const void* sr, const double* theta, const int* folds, int F, const Ws& cw,
                double* ghat, double* gvar, int ldo) {
    hipLaunchKernelGGL((cv_apply_kernel<T>), dim3((cw.n + TS - 1) / TS, cw.q), dim3(256), 0, st, (const T*)(cw.base + cw.off_V),
                       cw.mat, cw.npad, folds, F, w.q, (const T*)(w.base + w.off_b), (const T*)(w.base + w.off_z), w.npad,
                       (const T*)sr, theta, w.d + 3 + w.p, w.d, ldo, ghat, gvar);
    CHECK_LAUNCH("cv_apply_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Integrated variance reduction at fixed parameters (ALC / IMSPE reduction; no counterpart in the reference).  For
// reference points t, candidates c (standardised) and local component k, with U_k = (c0k o sr^T) L_k^-T as lcgp_predict forms it:
//     out[k, c] = sum_t w_t sigma_k(t, c)^2 / (max(gvar_k(c), 0) + 1 / (D_k r)),   sigma_k(t, c) = C_k(t, c) - D_k U_k(t) . U_k(c)
// (lcgp_hip.h).  lcgp_variance_reduction_prepare forms U_k of the reference set once; lcgp_variance_reduction forms U_k and gvar
// of a chunk of candidates (or takes them from the reference set), then ONE launch of the tile kernel (OP_VR: the n_ref x n_cand
// products stay in registers, the epilogue reduces them to one partial per reference tile) and vr_reduce_kernel.
// ---------------------------------------------------------------------------------------------------
constexpr int VR_XBLK = 2048;       // rows of X = c0k o sr^T formed per pass: bounds the X work area however large a set is

// scratch of the variance reduction: a reference part (offsets depend on n_ref only) followed by a candidate part (offsets
// relative to cand, from the n_cand of the call): a scratch sized for n_cand serves every call with fewer candidates
struct VrLay {
    int rrows, nrt, ldp, kp;
    size_t uslab_r, xslab_r, uslab_c, xslab_c;
    size_t off_uref, off_gvr, off_ghr, off_xr, off_str, cand;
    size_t off_uc, off_gvc, off_ghc, off_xc, off_stc, off_part, total;
};

// A conditioned view (lcgp_condition_prepare's state) the variance reduction and the selection run on instead of the fitted
// model (lcgp_condition_vr_* / lcgp_condition_select_*): rows of U are widened to K' = npad + mpad, [U_a | T_a / sqrt(D_k)],
// and gvar is the view's.  Everything behind the row former is the base model's code with K' as the row length.
struct VrView {
    const void* Un; const void* Wi; const void* xn;     // U_n and L_S^-1 of the state, the conditioning inputs
    int m, mpad;
};

// mpad > 0: the layout of a conditioned view -- rows of the two U are npad + mpad long, and each X work area is followed by
// the work area of Sigma_an and T (2 q rows mpad elements).  mpad = 0 is the base model's layout, byte for byte.
inline VrLay vr_carve(int dtype, int n, int q, int n_ref, int n_cand, int mpad = 0) {
    VrLay L;
    const size_t esz = dtype == LCGP_F64 ? 8 : 4, npad = round_up(n, 2 * TS), kp = npad + mpad;
    L.kp = (int)kp;
    // U_ref rows: whole 128-row tiles plus one 64-row tile, so that a candidate tile taken from ANY row of the reference set
    // (cand_row0 >= 0) stays inside the slab (its rows beyond the set only feed candidate columns that are never written)
    L.rrows = round_up(n_ref, 2 * TS) + TS;
    L.nrt = (n_ref + TS - 1) / TS;
    L.ldp = round_up(n_cand, TS);
    L.uslab_r = (size_t)L.rrows * kp;
    L.xslab_r = (size_t)min(VR_XBLK, predict_pad(n_ref)) * npad;
    size_t o = 0;
    L.off_uref = o; o = align256(o + (size_t)q * L.uslab_r * esz);
    L.off_gvr = o; o = align256(o + (size_t)q * n_ref * sizeof(double));
    L.off_ghr = o; o = align256(o + (size_t)q * n_ref * sizeof(double));
    L.off_xr = o; o = align256(o + (size_t)q * L.xslab_r * esz);
    L.off_str = o; o = align256(o + 2 * (size_t)q * min(VR_XBLK, predict_pad(n_ref)) * mpad * esz);
    L.cand = o;
    const int crows = predict_pad(n_cand);
    L.uslab_c = (size_t)crows * kp;
    L.xslab_c = (size_t)min(VR_XBLK, crows) * npad;
    L.off_uc = o; o = align256(o + (size_t)q * L.uslab_c * esz);
    L.off_gvc = o; o = align256(o + (size_t)q * n_cand * sizeof(double));
    L.off_ghc = o; o = align256(o + (size_t)q * n_cand * sizeof(double));
    L.off_xc = o; o = align256(o + (size_t)q * L.xslab_c * esz);
    L.off_stc = o; o = align256(o + 2 * (size_t)q * min(VR_XBLK, crows) * mpad * esz);
    L.off_part = o; o = align256(o + (size_t)q * L.nrt * L.ldp * sizeof(double));
    L.total = o;
    return L;
}

// U_k and gvar_k (ld = ldv per component) of m0 inputs xs for all local components, in passes of VR_XBLK rows: X = c0k o sr^T
// (cross_kernel, nugget term at column match[i] where given) into the X work area (q slabs xslab apart), U = X W^T (OP_PRED_U)
// into rows lo .. of the U slabs (uslab apart), then the row reductions (pred_reduce_kernel; gh receives ghat, unused).
// Per row the same arithmetic as lcgp_predict, whatever the pass.
// On a conditioned view (cv; ST: its work area of 2 q rows mpad elements) the rows of U are npad + mpad long, and each pass
// goes on with the launches of lcgp_condition_predict on its rows: the kernel values C^x(., xn), Sigma_an (OP_COND_CROSS, A rows
// npad + mpad apart), T = Sigma_an L_S^-T (OP_PRED_U on the dense L_S^-1), and cond_tail_kernel, which writes T / sqrt(D_k) behind
// the row's U and takes rowsum(T o T) off gvar: per row the arithmetic of lcgp_condition_predict.
template <typename T>
__global__ __launch_bounds__(64) void cond_tail_kernel(const T* __restrict__ Tm, size_t slab, int ld, int m, int mpad, int n0,
                                                       const double* __restrict__ theta, int tw, int d, T* __restrict__ Ut,
                                                       size_t uslab, int ldu, int ldo, double* __restrict__ gvar) {
    const int r = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    T* out = Ut + (size_t)k * uslab + (size_t)r * ldu;
    if (r >= n0) {                                  // (uniform per block) padding rows: zeros, whatever the scratch held
        for (int j = lane; j < mpad; j += 64) out[j] = (T)0;
        return;
    }
    const T* Tr = Tm + (size_t)k * slab + (size_t)r * ld;
    const double is = 1.0 / sqrt(theta[(size_t)k * tw + d + 2]);
    double s2 = 0.0;
    for (int j = lane; j < m; j += 64) {            // (cond_reduce_kernel's order)
        const double u = (double)Tr[j];
        s2 += u * u;
        out[j] = (T)(u * is);
    }
    for (int j = (m & ~63) + lane; j < mpad; j += 64)
        if (j >= m) out[j] = (T)0;                  // columns m .. mpad - 1: zeros, whatever T's padding held
    for (int off = 32; off > 0; off >>= 1) s2 += __shfl_xor(s2, off);
    if (lane == 0) gvar[(size_t)k * ldo + r] -= s2;
}

template <typename T>
int vr_form(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int m0, const void* xs,
            const int* match, T* X, size_t xslab, T* U, size_t uslab, double* gh, double* gv, int ldv,
            const VrView* cv = nullptr, T* ST = nullptr) {
    const int tw = w.d + 3 + w.p, ldu = w.npad + (cv ? cv->mpad : 0);
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for (int lo = 0; lo < m0; lo += VR_XBLK) {
        const int m = min(VR_XBLK, m0 - lo), mpad = predict_pad(m);
        const T* x0 = (const T*)xs + (size_t)lo * w.d;
        const int* mt = match ? match + lo : nullptr;
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(w.nb, mpad / TS, w.q), dim3(256), 0, st, X, w.npad, m,
                               w.n, w.d, x0, (const T*)x, dummy, theta, 0, (const T*)sr, mpad, w.npad, tw, xslab, mt);
        });
        CHECK_LAUNCH("cross_kernel");
        T* Ub = U + (size_t)lo * ldu;
        int rc = launch_pred<T, OP_PRED_U>(st, X, (const T*)(w.base + w.off_W), Ub, xslab, w.mat, w.npad, mpad, w.nb, w.q, uslab,
                                           false, ldu);
        if (rc) return rc;
        hipLaunchKernelGGL((pred_reduce_kernel<T>), dim3(m, w.q), dim3(64), 0, st, (const T*)X, (const T*)Ub, xslab, uslab, w.npad,
                           w.n, (const T*)(w.base + w.off_z), w.npad, theta, tw, w.d, ldv, gh + lo, gv + lo, ldu);
        CHECK_LAUNCH("pred_reduce_kernel");
        if (!cv) continue;
        const int cm = cv->mpad;
        const size_t cslab = (size_t)mpad * cm;
        T* Sg = ST;
        T* Tm = ST + cslab * w.q;
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(cm / TS, mpad / TS, w.q), dim3(256), 0, st, Sg, cm, m,
                               cv->m, w.d, x0, (const T*)cv->xn, dummy, theta, 0, (const T*)nullptr, mpad, cm, tw, cslab,
                               (const int*)nullptr);
        });
        CHECK_LAUNCH("cross_kernel");
        GemmArgs h;
        h.A = Ub; h.B = cv->Un; h.C = Sg;
        h.sA = uslab; h.sB = (size_t)cm * w.npad; h.sC = cslab; h.ldA = ldu; h.ldB = w.npad; h.ldC = cm;
        h.nb = 0; h.p0 = w.npad / TS; h.p1 = cm / TS; h.p2 = tw; h.p3 = w.d + 2;
        h.theta = theta;
        rc = launch_gemm<T, OP_COND_CROSS, 64>(st, h, (mpad / TS) * (cm / TS), w.q);
        if (rc) return rc;
        rc = launch_pred<T, OP_PRED_U>(st, Sg, (const T*)cv->Wi, Tm, cslab, (size_t)cm * cm, cm, mpad, cm / TS, w.q);
        if (rc) return rc;
        hipLaunchKernelGGL((cond_tail_kernel<T>), dim3(mpad, w.q), dim3(64), 0, st, (const T*)Tm, cslab, cm, cv->m, cm, m, theta, tw,
                           w.d, Ub + w.npad, uslab, ldu, ldv, gv + lo);
        CHECK_LAUNCH("cond_tail_kernel");
    }
    return 0;
}

template <typename T>
int do_vr_prepare(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n_ref, const void* x_ref,
                  char* scratch, const VrView* cv = nullptr) {
    const VrLay L = vr_carve(w.esz == 8 ? LCGP_F64 : LCGP_F32, w.n, w.q, n_ref, 1, cv ? cv->mpad : 0);
    return vr_form<T>(st, w, x, sr, theta, n_ref, x_ref, nullptr, (T*)(scratch + L.off_xr), L.xslab_r, (T*)(scratch + L.off_uref),
                      L.uslab_r, (double*)(scratch + L.off_ghr), (double*)(scratch + L.off_gvr), n_ref, cv,
                      (T*)(scratch + L.off_str));
}

// ---- joint posterior covariance of a conditioned view (lcgp_hip.h: lcgp_condition_predict_cov) ----
// Sigma'_k = C00_k - D_k U^ U^^T on the widened rows U^_a = [U_a | T_a / sqrt(D_k)] of all n0 new inputs: the row former above on a
// slab of n0pad x K' elements per component (n0pad = cov_pad(n0), what the factorisation expects), lcgp_predict_cov's prior,
// product (K = K') and diagonal.  scratch: the slab, the row former's two work areas, and the ghat / gvar it writes.
struct CondCovLay {
    int n0pad, mpad, kp, xb;        // xb: rows of a pass of the row former
    size_t uslab, xslab;
    size_t off_U, off_X, off_ST, off_gh, off_gv, total;
};

inline CondCovLay cond_cov_carve(int dtype, int n, int q, int m, int n0) {
    CondCovLay L;
    const size_t esz = dtype == LCGP_F64 ? 8 : 4, npad = round_up(n, 2 * TS);
    L.n0pad = cov_pad(n0);
    L.mpad = cov_pad(m);
    L.kp = (int)npad + L.mpad;
    L.xb = min(VR_XBLK, predict_pad(n0));
    L.uslab = (size_t)L.n0pad * L.kp;
    L.xslab = (size_t)L.xb * npad;
    size_t o = 0;
    L.off_U = o; o = align256(o + (size_t)q * L.uslab * esz);
    L.off_X = o; o = align256(o + (size_t)q * L.xslab * esz);
    L.off_ST = o; o = align256(o + 2 * (size_t)q * L.xb * L.mpad * esz);
    L.off_gh = o; o = align256(o + (size_t)q * n0 * sizeof(double));
    L.off_gv = o; o = align256(o + (size_t)q * n0 * sizeof(double));
    L.total = o;
    return L;
}

// zeroes count elements at U + k slab for every component k: the rows of the slab behind the last pass of the row former
template <typename T>
__global__ __launch_bounds__(256) void cond_cov_zero_kernel(T* __restrict__ U, size_t slab, size_t count) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) U[(size_t)blockIdx.y * slab + e] = (T)0;
}

template <typename T>
int do_condition_predict_cov(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const VrView& cv,
                             int n0, const void* x0, char* scratch, const Ws& cw, double jitter) {
    const CondCovLay L = cond_cov_carve(sizeof(T) == 4 ? LCGP_F32 : LCGP_F64, w.n, w.q, cv.m, n0);
    const int n0pad = L.n0pad, tw = w.d + 3 + w.p;
    T* U = (T*)(scratch + L.off_U);
    T* M = (T*)(cw.base + cw.off_M);
    // the widened rows of all n0 inputs, no match term (same = 0: the continuous surface, also at training inputs and at the
    // view's own inputs)
    int rc = vr_form<T>(st, w, x, sr, theta, n0, x0, nullptr, (T*)(scratch + L.off_X), L.xslab, U, L.uslab,
                        (double*)(scratch + L.off_gh), (double*)(scratch + L.off_gv), n0, &cv, (T*)(scratch + L.off_ST));
    if (rc) return rc;
    // the row former pads a last pass of fewer than 128 rows to 64, the slab is padded to 128: up to 64 rows behind it were not
    // written, and the product reads them
    const int rem = n0 % VR_XBLK, done = n0 - rem + (rem ? predict_pad(rem) : 0);
    if (done < n0pad) {
        const size_t count = (size_t)(n0pad - done) * L.kp;
        hipLaunchKernelGGL((cond_cov_zero_kernel<T>), dim3((unsigned)((count + 255) / 256), w.q), dim3(256), 0, st,
                           U + (size_t)done * L.kp, L.uslab, count);
        CHECK_LAUNCH("cond_cov_zero_kernel");
    }
    // the prior C00 with the nugget on its diagonal, as do_predict_cov writes it
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<T, decltype(kern)::value>), dim3(n0pad / TS, n0pad / TS, w.q), dim3(256), 0, st, M, n0pad,
                           n0, n0, w.d, (const T*)x0, (const T*)x0, dummy, theta, 1, (const T*)nullptr, n0pad, n0pad, tw, cw.mat,
                           (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    GemmArgs h;
    h.A = U; h.B = U; h.C = M;
    h.sA = h.sB = L.uslab; h.sC = cw.mat; h.ldA = h.ldB = L.kp; h.ldC = n0pad;
    h.p1 = tw; h.p2 = w.d + 2; h.p3 = 0;
    h.theta = theta;
    const int t64 = n0pad / TS;         // (64x64 tiles: do_predict_cov)
    h.nb = t64; h.p0 = L.kp / TS;
    rc = launch_gemm<T, OP_PRED_COV, 64>(st, h, t64 * (t64 + 1) / 2, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL((cov_diag_kernel<T>), dim3((n0pad + 255) / 256, w.q), dim3(256), 0, st, M, cw.mat, n0, n0pad, theta, tw,
                       w.d, jitter);
    CHECK_LAUNCH("cov_diag_kernel");
    return 0;
}

// out[k, c] = sum over the reference tiles, in ascending order, of the partials the OP_VR epilogue left
__global__ __launch_bounds__(256) void vr_reduce_kernel(const double* __restrict__ part, int nrt, int ldp, int n_cand, int ldo,
                                                        double* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (c >= n_cand) return;
    const double* pk = part + (size_t)k * nrt * ldp + c;
    double s = 0.0;
    for (int rt = 0; rt < nrt; ++rt) s += pk[(size_t)rt * ldp];
    out[(size_t)k * ldo + c] = s;
}

template <typename T>
int do_vr(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n_ref, const void* x_ref,
          const double* w_ref, int n_cand, const void* x_cand, const int* match, int row0, int r, char* scratch, double* out,
          int ldo, const VrView* cv = nullptr) {
    const VrLay L = vr_carve(w.esz == 8 ? LCGP_F64 : LCGP_F32, w.n, w.q, n_ref, n_cand, cv ? cv->mpad : 0);
    const T* Ur = (const T*)(scratch + L.off_uref);
    const T* Uc;
    const double* gvc;
    const void* xc;
    size_t sB;
    int ldg;
    if (row0 >= 0) {                // the candidates are rows row0 .. of the reference set: its U and gvar serve
        Uc = Ur + (size_t)row0 * L.kp; sB = L.uslab_r;
        gvc = (const double*)(scratch + L.off_gvr) + row0; ldg = n_ref;
        xc = (const T*)x_ref + (size_t)row0 * w.d;
    } else {
        T* U = (T*)(scratch + L.off_uc);
        double* gv = (double*)(scratch + L.off_gvc);
        int rc = vr_form<T>(st, w, x, sr, theta, n_cand, x_cand, match, (T*)(scratch + L.off_xc), L.xslab_c, U, L.uslab_c,
                            (double*)(scratch + L.off_ghc), gv, n_cand, cv, (T*)(scratch + L.off_stc));
        if (rc) return rc;
        Uc = U; sB = L.uslab_c; gvc = gv; ldg = n_cand; xc = x_cand;
    }
    GemmArgs h;
    h.A = Ur; h.B = Uc; h.C = scratch + L.off_part;
    h.sA = L.uslab_r; h.sB = sB; h.sC = 0;
    h.ldA = h.ldB = L.kp; h.ldC = 0;                // (a conditioned view: the widened rows, K = npad + mpad)
    h.nb = 0;
    h.p0 = L.kp / TS; h.p1 = (n_cand + TS - 1) / TS; h.p2 = n_ref; h.p3 = n_cand;
    h.theta = theta; h.xa = x_ref; h.xb = xc; h.wref = w_ref; h.gvc = gvc; h.ldg = ldg;
    h.d = w.d; h.kern = w.kern; h.tw = w.d + 3 + w.p; h.nrep = r; h.ldp = L.ldp;
    // 64x64 tiles: the 128-tile instances of the U U^T product do not compile clean (OP_PRED_COV), and this
    // epilogue holds more than that one's
    int rc = launch_gemm<T, OP_VR, 64>(st, h, L.nrt * h.p1, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL(vr_reduce_kernel, dim3((n_cand + 255) / 256, w.q), dim3(256), 0, st,
                       (const double*)(scratch + L.off_part), L.nrt, L.ldp, n_cand, ldo, out);
    CHECK_LAUNCH("vr_reduce_kernel");
    return 0;
}

// host-side checks of the variance-reduction arguments shared by the two entries
int check_vr(int n_ref, int n_cand) {
    if (n_ref < 1) return bad("n_ref must be >= 1");
    if (n_cand < 1) return bad("n_cand must be >= 1");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Gradient of the integrated variance reduction with respect to the candidate (lcgp_hip.h: lcgp_variance_reduction_grad; no
// counterpart in the reference).  With R = N / den as above, every candidate a new input, S[c, t] = w_t sigma(t, c):
//     d_l R(c) = (d_l N - R d_l h) / den          d_l h = -2 D sum_j dc_l(c, j) sr_j V[c, j]   (pgrad_kernel's dgvar; 0 where h <= 0)
//     d_l N(c) = 2 [ sum_t dC_l(c, t) S[c, t]  -  D sum_j dc_l(c, j) sr_j Q[c, j] ],      Q = (S U_ref) W,   V = U_cand W
// R comes from do_vr itself (bitwise lcgp_variance_reduction).  Then P = U_cand U_ref^T (OP_VG_P, the product OP_VR keeps in
// registers), S from P in place (vrg_sigma_kernel: C recomputed in double as the OP_VR epilogue forms it), the first sum by the
// fused contraction over the REFERENCE points (pgrad_kernel<ZMAT> with z = S), G = S U_ref (OP_VG_G), Q and V (OP_PRED_V), the
// other two sums by ONE contraction over the training inputs (pgrad_kernel<ZMAT> with z = Q beside V), and vrg_combine_kernel.
// Every row of every product depends on its candidate only, every sum has a fixed order: bitwise independent of q_local, of
// the scratch content and of how the candidates are split over calls.
// ---------------------------------------------------------------------------------------------------
struct VrgLay {
    int crows, lds;                 // rows of the candidate slabs; row length of S (n_ref rounded up to 128)
    size_t sslab, gslab, qslab, nslab;
    size_t off_s, off_g, off_q, off_t, off_a, off_h, off_u, off_qn, off_rc, total;    // relative to the end of the variance
                                                                                      // reduction's own scratch
};

// mpad > 0: the layout of a conditioned view (lcgp_condition_vr_grad) -- the rows of G are npad + mpad long (gslab), and behind
// the base layout lie U' (rows npad long, qslab) and Q_n, R_c (rows mpad long, nslab).  mpad = 0 is the base model's layout,
// byte for byte.
inline VrgLay vrg_carve(int dtype, int n, int d, int q, int n_ref, int n_cand, int mpad = 0) {
    VrgLay G;
    const size_t esz = dtype == LCGP_F64 ? 8 : 4, npad = round_up(n, 2 * TS);
    G.crows = predict_pad(n_cand);
    G.lds = round_up(n_ref, 2 * TS);
    G.sslab = (size_t)G.crows * G.lds;
    G.gslab = (size_t)G.crows * (npad + mpad);
    G.qslab = (size_t)G.crows * npad;
    G.nslab = (size_t)G.crows * mpad;
    size_t o = 0;
    G.off_s = o; o = align256(o + (size_t)q * G.sslab * esz);
    G.off_g = o; o = align256(o + (size_t)q * G.gslab * esz);
    G.off_q = o; o = align256(o + (size_t)q * G.qslab * esz);
    G.off_t = o; o = align256(o + (size_t)q * n_cand * d * sizeof(double));
    G.off_a = o; o = align256(o + (size_t)q * n_cand * d * sizeof(double));
    G.off_h = o; o = align256(o + (size_t)q * n_cand * d * sizeof(double));
    G.off_u = o; o = align256(o + (mpad ? (size_t)q * G.qslab * esz : 0));
    G.off_qn = o; o = align256(o + (size_t)q * G.nslab * esz);
    G.off_rc = o; o = align256(o + (size_t)q * G.nslab * esz);
    G.total = o;
    return G;
}

// S[k, c, t] = w_t (C_k(c, t) - D_k P[k, c, t]) in place over P (row length lds), zero beyond n_cand rows / n_ref columns (the
// k padding of S U_ref).  C_k in double from the standardised inputs divided by ell, the arithmetic of the OP_VR epilogue.
template <typename T, int KERN>
__global__ __launch_bounds__(256) void vrg_sigma_kernel(T* __restrict__ S, size_t sslab, int lds, int n_cand, int n_ref, int d,
                                                        const T* __restrict__ xc, const T* __restrict__ xr,
                                                        const double* __restrict__ wref, const double* __restrict__ theta, int tw) {
    const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, k = blockIdx.z;
    if (t >= lds) return;
    T* p = S + (size_t)k * sslab + (size_t)c * lds + t;
    if (c >= n_cand || t >= n_ref) { *p = (T)0; return; }
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double coff = scale * (1.0 - nug / (1.0 + nug));
    double poly = 1.0, ssum = 0.0;
    for (int l = 0; l < d; ++l) {
        const double xv = (double)xr[(size_t)t * d + l] / th[l], yv = (double)xc[(size_t)c * d + l] / th[l];
        if constexpr (KERN == 0) {
            const double sd = fabs(xv - yv);
            poly = fma(poly, sd, poly);
            ssum -= sd;
        } else if constexpr (KERN == 1) {
            const double df = xv - yv;
            ssum = fma(-0.5 * df, df, ssum);
        } else {
            static_assert(KERN == 2, "unknown covariance kernel id");
            const double sd = fabs(xv - yv);
            poly = fma(poly, m52_fm1(sd), poly);
            ssum -= sd;
        }
    }
    const double sg = fma(-D, (double)*p, coff * kern_c0<KERN>(poly, ssum));
    *p = (T)(wref[t] * sg);
}

// dR[k, c, l] = (2 (t1 - D_k a1) - R_k(c) dh) / den_c; dh counts only where the candidate's gvar is positive
// COND (a conditioned view): a1 arrives with D_k on its first segment's weights, 2 (t1 - a1)
template <bool COND>
__global__ __launch_bounds__(256) void vrg_combine_kernel(const double* __restrict__ R, int ldo, const double* __restrict__ gvc, int ldg,
                                                          const double* __restrict__ theta, int tw, int d, int nrep, int n_cand,
                                                          const double* __restrict__ t1, const double* __restrict__ a1,
                                                          const double* __restrict__ dh, double* __restrict__ dR) {
    const int e = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (e >= n_cand * d) return;
    const int c = e / d;
    const double D = theta[(size_t)k * tw + d + 2];
    const double h = gvc[(size_t)k * ldg + c];
    const double den = fmax(h, 0.0) + 1.0 / (D * (double)nrep);
    const size_t io = (size_t)k * ldo * d + e, is = (size_t)k * n_cand * d + e;
    const double dhv = h > 0.0 ? dh[is] : 0.0;
    const double num = COND ? t1[is] - a1[is] : fma(-D, a1[is], t1[is]);
    dR[io] = (2.0 * num - R[(size_t)k * ldo + c] * dhv) / den;
}

// a conditioned view: dst[k, r, j] = f_k src[k, r, j] for r < rows, j < cols (rows lds / ldd apart, slabs sslab / dslab apart),
// f_k = sqrt(D_k) (scale: the tails T / sqrt(D_k) of the widened rows back to T's scale) or 1 (a copy)
template <typename T>
__global__ __launch_bounds__(256) void vrg_rows_kernel(const T* __restrict__ src, size_t sslab, int lds, T* __restrict__ dst,
                                                       size_t dslab, int ldd, int cols, int scale,
                                                       const double* __restrict__ theta, int tw, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, k = blockIdx.z;
    if (j >= cols) return;
    const T v = src[(size_t)k * sslab + (size_t)r * lds + j];
    dst[(size_t)k * dslab + (size_t)r * ldd + j] = scale ? (T)((double)v * sqrt(theta[(size_t)k * tw + d + 2])) : v;
}

// the fused contraction with a matrix in the place of z (outputs n0 rows apart per component)
template <typename T>
int launch_pgrad_mat(hipStream_t st, const Ws& w, const void* x0, int n0, const void* x, const void* sr, int n,
                     const double* theta, const T* Z, const T* V, int ld, size_t slab, double* dz, double* dv) {
    const int wide = w.d > 16;
    dim3 grid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, wide ? (w.d + DMAX - 1) / DMAX : 1);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((pgrad_kernel<T, decltype(dd)::value, decltype(kern)::value, true>), grid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, n, w.d, theta, w.d + 3 + w.p, Z, ld, V, slab, n0, dz, dv);
        });
    });
    CHECK_LAUNCH("pgrad_kernel");
    return 0;
}

// the same contraction on a conditioned view: over the n + m columns, Z beside V (rows npad long, slabs `slab` apart) and Zn
// beside Rn (rows mpad long, slabs `nslab` apart)
template <typename T>
int launch_pgrad_cond_mat(hipStream_t st, const Ws& w, const void* x0, int n0, const void* x, const void* sr, const double* theta,
                          const T* Z, const T* V, size_t slab, const VrView& cv, const T* Zn, const T* Rn, size_t nslab,
                          double* dz, double* dv) {
    PgradCond<T> cs;
    cs.zd = nullptr; cs.wv = nullptr;
    cs.xn = (const T*)cv.xn; cs.m = cv.m; cs.mpad = cv.mpad;
    cs.R = Rn; cs.rslab = nslab;
    const int wide = w.d > 16;
    dim3 grid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, wide ? (w.d + DMAX - 1) / DMAX : 1);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((pgrad_cond_mat_kernel<T, decltype(dd)::value, decltype(kern)::value>), grid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, w.n, w.d, theta, w.d + 3 + w.p, Z, w.npad, V, slab, n0,
                               dz, dv, cs, Zn);
        });
    });
    CHECK_LAUNCH("pgrad_cond_mat_kernel");
    return 0;
}

// On a conditioned view (cv; lcgp_condition_vr_grad) the rows of the two U are the widened rows U^ = [U | T / sqrt(D)] of length
// K' = npad + mpad: P' = U^_cand U^_ref^T and S' as above, G^ = S' U^_ref = [G_U | G_T / sqrt(D)] over K' columns, then with the
// state's dense L_S^-1 and U_n (the notation of lcgp_condition_predict_grad)
//     Q_n = G_T L_S^-1,   Q' = (G_U - Q_n U_n) W,   R_c = T_c L_S^-1,   V'_c = (U_c - R_c U_n) W
//     a1 = D sum_j dc_l sr_j Q' + sum_a dc^x_l Q_n,     d_l h' = -2 D sum_j dc_l sr_j V'_c - 2 sum_a dc^x_l R_c,
//     d_l R' = (2 (t1 - a1) - R' d_l h') / den'
// by ONE contraction over the n + m columns (pgrad_cond_mat_kernel).  U_c - R_c U_n goes into a buffer of its own: the
// candidates' rows may be rows of U^_ref.
template <typename T>
int do_vr_grad(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n_ref, const void* x_ref,
               const double* w_ref, int n_cand, const void* x_cand, int row0, int r, char* scratch, double* out, int ldo,
               double* dout, const VrView* cv = nullptr) {
    const int dt = w.esz == 8 ? LCGP_F64 : LCGP_F32, mpad = cv ? cv->mpad : 0;
    const VrLay L = vr_carve(dt, w.n, w.q, n_ref, n_cand, mpad);
    const VrgLay G = vrg_carve(dt, w.n, w.d, w.q, n_ref, n_cand, mpad);
    const int kp = L.kp, tw = w.d + 3 + w.p;
    int rc = do_vr<T>(st, w, x, sr, theta, n_ref, x_ref, w_ref, n_cand, x_cand, nullptr, row0, r, scratch, out, ldo, cv);
    if (rc) return rc;
    // U, gvar and inputs of the candidates, where do_vr left or found them
    T* Ur = (T*)(scratch + L.off_uref);
    const T* Uc;
    const double* gvc;
    const void* xc;
    size_t sUc;
    int ldg, rows;
    if (row0 >= 0) {
        // rows of the reference set: whole 64-tiles only, which stay inside its slab (vr_carve)
        Uc = Ur + (size_t)row0 * kp; sUc = L.uslab_r; rows = round_up(n_cand, TS);
        gvc = (const double*)(scratch + L.off_gvr) + row0; ldg = n_ref;
        xc = (const T*)x_ref + (size_t)row0 * w.d;
    } else {
        Uc = (const T*)(scratch + L.off_uc); sUc = L.uslab_c; rows = G.crows;
        gvc = (const double*)(scratch + L.off_gvc); ldg = n_cand; xc = x_cand;
    }
    char* ex = scratch + L.total;
    T* S = (T*)(ex + G.off_s);
    T* Gb = (T*)(ex + G.off_g);
    T* Qb = (T*)(ex + G.off_q);
    double* t1 = (double*)(ex + G.off_t);
    double* a1 = (double*)(ex + G.off_a);
    double* dh = (double*)(ex + G.off_h);
    // the rows of U_ref between the set and the k padding of S U_ref: zeros (those up to the padding of the passes that formed
    // the set are zeros already; the rest has never been written)
    if (G.lds > n_ref) {
        hipError_t e = hipMemset2DAsync(Ur + (size_t)n_ref * kp, L.uslab_r * w.esz, 0,
                                        (size_t)(G.lds - n_ref) * kp * w.esz, w.q, st);
        if (e != hipSuccess) return fail("hipMemset2DAsync", e);
    }
    GemmArgs h;
    h.A = Uc; h.B = Ur; h.C = S;
    h.sA = sUc; h.sB = L.uslab_r; h.sC = G.sslab;
    h.ldA = h.ldB = kp; h.ldC = G.lds;
    h.nb = 0; h.p0 = kp / TS; h.p1 = G.lds / TS; h.p2 = h.p3 = 0;
    rc = launch_gemm<T, OP_VG_P, 64>(st, h, (rows / TS) * h.p1, w.q);
    if (rc) return rc;
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((vrg_sigma_kernel<T, decltype(kern)::value>), dim3((G.lds + 255) / 256, rows, w.q), dim3(256), 0, st, S,
                           G.sslab, G.lds, n_cand, n_ref, w.d, (const T*)xc, (const T*)x_ref, w_ref, theta, tw);
    });
    CHECK_LAUNCH("vrg_sigma_kernel");
    // t1[c, l] = sum_t dC_l(c, t) S[c, t]   (a1 receives the same sum scaled: overwritten below)
    rc = launch_pgrad_mat<T>(st, w, xc, n_cand, x_ref, nullptr, n_ref, theta, S, S, G.lds, G.sslab, t1, a1);
    if (rc) return rc;
    GemmArgs g;
    g.A = S; g.B = Ur; g.C = Gb;
    g.sA = G.sslab; g.sB = L.uslab_r; g.sC = G.gslab;
    g.ldA = G.lds; g.ldB = g.ldC = kp; g.p2 = g.p3 = 0;
    // 64x64 tiles for G, Q and V whatever the number of candidates: OP_PRED_V sums in a different order on 128-row tiles
    // (DESIGN 4.2), and a call's candidates may be any rows of a larger set
    g.nb = kp / TS; g.p0 = rows / TS; g.p1 = G.lds / TS;
    rc = launch_gemm<T, OP_VG_G, 64>(st, g, g.p0 * g.nb, w.q);
    if (rc) return rc;
    const T* W = (const T*)(w.base + w.off_W);
    if (!cv) {
        rc = launch_pred<T, OP_PRED_V>(st, Gb, W, Qb, G.gslab, w.mat, w.npad, rows, w.nb, w.q, 0, true);
        if (rc) return rc;
        rc = launch_pred<T, OP_PRED_V>(st, Uc, W, Gb, sUc, w.mat, w.npad, rows, w.nb, w.q, G.gslab, true); // (G is free: V = U_cand W)
        if (rc) return rc;
        rc = launch_pgrad_mat<T>(st, w, xc, n_cand, x, sr, w.n, theta, Qb, Gb, w.npad, G.gslab, a1, dh);
        if (rc) return rc;
        hipLaunchKernelGGL(vrg_combine_kernel<false>, dim3((n_cand * w.d + 255) / 256, w.q), dim3(256), 0, st, (const double*)out,
                           ldo, gvc, ldg, theta, tw, w.d, r, n_cand, (const double*)t1, (const double*)a1, (const double*)dh, dout);
        CHECK_LAUNCH("vrg_combine_kernel");
        return 0;
    }
    T* Up = (T*)(ex + G.off_u);
    T* Qn = (T*)(ex + G.off_qn);
    T* Rc = (T*)(ex + G.off_rc);
    const T* Wi = (const T*)cv->Wi;
    const T* Un = (const T*)cv->Un;
    const size_t wimat = (size_t)mpad * mpad, unmat = (size_t)mpad * w.npad;
    const dim3 tgrid((mpad + 255) / 256, rows, w.q), ugrid((w.npad + 255) / 256, rows, w.q);
    // `tails` = the mpad columns behind the npad of a widened row, times L_S^-1 (OP_PRED_V on the dense L_S^-1, rows K' apart in,
    // mpad apart out), then to T's scale; `minus_un` = C - A U_n in place (OP_COND_U, K = mpad); `times_w` = A W (OP_PRED_V)
    auto tails = [&](const T* A, size_t sA, T* C) -> int {
        GemmArgs a;
        a.A = A + w.npad; a.B = Wi; a.C = C;
        a.sA = sA; a.sB = wimat; a.sC = G.nslab; a.ldA = kp; a.ldB = a.ldC = mpad; a.p1 = a.p2 = a.p3 = 0;
        a.nb = mpad / TS; a.p0 = rows / TS;
        int e = launch_gemm<T, OP_PRED_V, 64>(st, a, a.p0 * a.nb, w.q);
        if (e) return e;
        hipLaunchKernelGGL((vrg_rows_kernel<T>), tgrid, dim3(256), 0, st, (const T*)C, G.nslab, mpad, C, G.nslab, mpad, mpad, 1, theta,
                           tw, w.d);
        CHECK_LAUNCH("vrg_rows_kernel");
        return 0;
    };
    auto minus_un = [&](const T* A, T* C, size_t sC, int ldC) -> int {
        GemmArgs a;
        a.A = A; a.B = Un; a.C = C;
        a.sA = G.nslab; a.sB = unmat; a.sC = sC; a.ldA = mpad; a.ldB = w.npad; a.ldC = ldC; a.p2 = a.p3 = 0;
        a.nb = w.nb; a.p0 = rows / TS; a.p1 = mpad / TS;
        return launch_gemm<T, OP_COND_U, 64>(st, a, a.p0 * a.nb, w.q);
    };
    auto times_w = [&](const T* A, size_t sA, int ldA, T* C) -> int {
        GemmArgs a;
        a.A = A; a.B = W; a.C = C;
        a.sA = sA; a.sB = w.mat; a.sC = G.qslab; a.ldA = ldA; a.ldB = a.ldC = w.npad; a.p1 = a.p2 = a.p3 = 0;
        a.nb = w.nb; a.p0 = rows / TS;
        return launch_gemm<T, OP_PRED_V, 64>(st, a, a.p0 * a.nb, w.q);
    };
    // Q_n = G_T L_S^-1,  Q' = (G_U - Q_n U_n) W
    if ((rc = tails(Gb, G.gslab, Qn))) return rc;
    if ((rc = minus_un(Qn, Gb, G.gslab, kp))) return rc;
    if ((rc = times_w(Gb, G.gslab, kp, Qb))) return rc;
    // R_c = T_c L_S^-1,  V'_c = (U_c - R_c U_n) W into the slab of G (free now; rows npad long)
    if ((rc = tails(Uc, sUc, Rc))) return rc;
    hipLaunchKernelGGL((vrg_rows_kernel<T>), ugrid, dim3(256), 0, st, Uc, sUc, kp, Up, G.qslab, w.npad, w.npad, 0, theta, tw, w.d);
    CHECK_LAUNCH("vrg_rows_kernel");
    if ((rc = minus_un(Rc, Up, G.qslab, w.npad))) return rc;
    if ((rc = times_w(Up, G.qslab, w.npad, Gb))) return rc;
    rc = launch_pgrad_cond_mat<T>(st, w, xc, n_cand, x, sr, theta, Qb, Gb, G.qslab, *cv, Qn, Rc, G.nslab, a1, dh);
    if (rc) return rc;
    hipLaunchKernelGGL(vrg_combine_kernel<true>, dim3((n_cand * w.d + 255) / 256, w.q), dim3(256), 0, st, (const double*)out, ldo,
                       gvc, ldg, theta, tw, w.d, r, n_cand, (const double*)t1, (const double*)a1, (const double*)dh, dout);
    CHECK_LAUNCH("vrg_combine_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Greedy batch design by sequential ALC (lcgp_hip.h: lcgp_select_*; no counterpart in the reference).  The state per local
// component is R(c) = N(c) / den(c) (what lcgp_variance_reduction writes), h(c) (the candidates' gvar) and the history rows
// V[s, :] (candidates) / Uh[s, :] (reference points) of the picks made so far: a pivoted Cholesky of the posterior covariance
// over the candidates carried lazily.  A step streams U_cand and U_ref twice each; nothing of size n_ref x n_cand is stored.
// The step kernels are bandwidth-bound row passes: one wave per row of U, 16-byte loads, double sums in a fixed order.
// ---------------------------------------------------------------------------------------------------
constexpr int SEL_RB = 32;          // reference rows per partial of the transposed product (fixed: results do not depend on sizes)

struct SelLay {
    int rrows, crows, xrows, nrt, ldp, nchunk, kp;
    size_t uslab_r, uslab_c, xslab;
    size_t off_uref, off_gvr, off_ghr, off_x, off_st, off_uc, off_ghc, off_h, off_part, off_R, off_V, off_Uh, off_ypart, off_y, off_b,
        off_xsr, off_xsc, off_w, off_mask, off_picks, total;
};

// (mpad > 0: the layout of a conditioned view, as vr_carve's -- rows of npad + mpad, the Sigma_an / T work area behind X)
inline SelLay sel_carve(int dtype, int n, int d, int q, int n_ref, int n_cand, int size, int mpad = 0) {
    SelLay L;
    const size_t esz = dtype == LCGP_F64 ? 8 : 4, npad = round_up(n, 2 * TS), kp = npad + mpad;
    L.kp = (int)kp;
    L.rrows = round_up(n_ref, 2 * TS) + TS;                 // as VrLay
    L.crows = predict_pad(n_cand) + 2 * TS;                 // the last pass of lcgp_select_begin writes whole tiles past n_cand
    L.xrows = min(VR_XBLK, max(predict_pad(n_ref), predict_pad(n_cand)));
    L.nrt = (n_ref + TS - 1) / TS;
    L.ldp = round_up(n_cand, TS);
    L.nchunk = (n_ref + SEL_RB - 1) / SEL_RB;
    L.uslab_r = (size_t)L.rrows * kp;
    L.uslab_c = (size_t)L.crows * kp;
    L.xslab = (size_t)L.xrows * npad;
    const size_t D8 = sizeof(double);
    size_t o = 0;
    L.off_uref = o; o = align256(o + (size_t)q * L.uslab_r * esz);
    L.off_uc = o; o = align256(o + (size_t)q * L.uslab_c * esz);
    L.off_x = o; o = align256(o + (size_t)q * L.xslab * esz);
    L.off_st = o; o = align256(o + 2 * (size_t)q * L.xrows * mpad * esz);
    L.off_gvr = o; o = align256(o + (size_t)q * n_ref * D8);
    L.off_ghr = o; o = align256(o + (size_t)q * n_ref * D8);
    L.off_ghc = o; o = align256(o + (size_t)q * n_cand * D8);
    L.off_h = o; o = align256(o + (size_t)q * n_cand * D8);
    L.off_part = o; o = align256(o + (size_t)q * L.nrt * L.ldp * D8);
    L.off_R = o; o = align256(o + (size_t)q * n_cand * D8);
    L.off_V = o; o = align256(o + (size_t)q * size * n_cand * D8);
    L.off_Uh = o; o = align256(o + (size_t)q * size * n_ref * D8);
    L.off_ypart = o; o = align256(o + (size_t)q * L.nchunk * kp * D8);
    L.off_y = o; o = align256(o + (size_t)q * kp * D8);
    L.off_b = o; o = align256(o + (size_t)q * size * D8);
    L.off_xsr = o; o = align256(o + (size_t)q * n_ref * d * D8);
    L.off_xsc = o; o = align256(o + (size_t)q * n_cand * d * D8);
    L.off_w = o; o = align256(o + (size_t)n_ref * D8);
    L.off_mask = o; o = align256(o + (size_t)n_cand * sizeof(int));
    L.off_picks = o; o = align256(o + (size_t)size * sizeof(int));
    L.total = o;
    return L;
}

// sums over the 64 lanes in a fixed order; every lane returns the total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// 16 bytes of a row: VEC = 2 doubles or 4 floats
template <typename T> struct SelVec;
template <> struct SelVec<double> { typedef double v __attribute__((ext_vector_type(2))); static constexpr int N = 2; };
template <> struct SelVec<float> { typedef float v __attribute__((ext_vector_type(4))); static constexpr int N = 4; };

// a . b over k < n for two rows of a U slab (16-byte aligned: rows are npad apart), double accumulation; one wave, every lane
// returns the sum.  Lane l takes the 16-byte pieces l, l + 64, ..
template <typename T>
__device__ __forceinline__ double sel_row_dot(const T* __restrict__ a, const T* __restrict__ b, int n, int lane) {
    constexpr int VN = SelVec<T>::N;
    typedef typename SelVec<T>::v V;
    double acc = 0.0;
    const int nv = n / VN;
#pragma unroll 4
    for (int i = lane; i < nv; i += 64) {
        const V x = *(const V*)(a + (size_t)i * VN), y = *(const V*)(b + (size_t)i * VN);
#pragma unroll
        for (int e = 0; e < VN; ++e) acc = fma((double)x[e], (double)y[e], acc);
    }
    const int tail = nv * VN + lane;
    if (tail < n) acc = fma((double)a[tail], (double)b[tail], acc);
    return wave_sum(acc);
}

// the same with a double vector y as the second operand
template <typename T>
__device__ __forceinline__ double sel_row_dot_y(const T* __restrict__ a, const double* __restrict__ y, int n, int lane) {
    constexpr int VN = SelVec<T>::N;
    typedef typename SelVec<T>::v V;
    typedef SelVec<double>::v D2;
    double acc = 0.0;
    const int nv = n / VN;
#pragma unroll 4
    for (int i = lane; i < nv; i += 64) {
        const V x = *(const V*)(a + (size_t)i * VN);
#pragma unroll
        for (int e = 0; e < VN; e += 2) {
            const D2 yy = *(const D2*)(y + (size_t)i * VN + e);
            acc = fma((double)x[e], yy[0], acc);
            acc = fma((double)x[e + 1], yy[1], acc);
        }
    }
    const int tail = nv * VN + lane;
    if (tail < n) acc = fma((double)a[tail], y[tail], acc);
    return wave_sum(acc);
}

// the product kernel (without scale and nugget) of two inputs already divided by ell, as cross_kernel forms it
template <int KERN>
__device__ __forceinline__ double sel_kern(const double* __restrict__ a, const double* __restrict__ b, int d) {
    double pl = 1.0, ss = 0.0;
    for (int l = 0; l < d; ++l) {
        if constexpr (KERN == 0) {
            const double sd = fabs(a[l] - b[l]);
            pl = fma(pl, sd, pl);
            ss -= sd;
        } else if constexpr (KERN == 1) {
            const double df = a[l] - b[l];
            ss = fma(-0.5 * df, df, ss);
        } else {
            static_assert(KERN == 2, "unknown covariance kernel id");
            const double sd = fabs(a[l] - b[l]);
            pl = fma(pl, m52_fm1(sd), pl);
            ss -= sd;
        }
    }
    return kern_c0<KERN>(pl, ss);
}

// xs[k, i, l] = x[i, l] / ell_k[l] in double
template <typename T>
__global__ __launch_bounds__(256) void sel_scale_kernel(const T* __restrict__ x, int m, int d, const double* __restrict__ theta,
                                                        int tw, double* __restrict__ xs) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (e >= m * d) return;
    xs[(size_t)k * m * d + e] = (double)x[e] / theta[(size_t)k * tw + (e % d)];
}

__global__ __launch_bounds__(256) void sel_init_kernel(const double* __restrict__ w_in, int n_ref, double* __restrict__ w,
                                                       int n_cand, int* __restrict__ mask, int size, int* __restrict__ picks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ref) w[i] = w_in[i];
    if (i < n_cand) mask[i] = 0;
    if (i < size) picks[i] = 0;
}

// (i) the current covariance column of pick j over candidates and reference points, scaled:
//   row c < n_cand:  V[t, c]  = (C^x(c, j) - D U_cand(c) . U_cand(j) - sum_{s<t} V[s, c]  V[s, j]) / sqrt(den_j)
//   row n_cand + r:  Uh[t, r] = (C^x(r, j) - D U_ref(r)  . U_cand(j) - sum_{s<t} Uh[s, r] V[s, j]) / sqrt(den_j)
// one wave per row, four rows per workgroup
template <typename T, int KERN>
__global__ __launch_bounds__(256) void sel_col_kernel(const T* __restrict__ Uc, size_t sUc, const T* __restrict__ Ur, size_t sUr,
                                                      int npad, int n, int n_cand, int n_ref, const double* __restrict__ xsc,
                                                      const double* __restrict__ xsr, int d, const double* __restrict__ theta,
                                                      int tw, int nrep, const double* __restrict__ h, double* __restrict__ V,
                                                      double* __restrict__ Uh, int size, int t, const int* __restrict__ pick) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), k = blockIdx.y;
    if (row >= n_cand + n_ref) return;                      // (uniform per wave)
    const int j = *pick;
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double coff = scale * (1.0 - nug / (1.0 + nug));
    const bool isc = row < n_cand;
    const int r = isc ? row : row - n_cand;
    const T* __restrict__ a = isc ? Uc + (size_t)k * sUc + (size_t)r * npad : Ur + (size_t)k * sUr + (size_t)r * npad;
    const T* __restrict__ b = Uc + (size_t)k * sUc + (size_t)j * npad;
    const double dot = sel_row_dot<T>(a, b, n, lane);
    const double* xr = isc ? xsc + ((size_t)k * n_cand + r) * d : xsr + ((size_t)k * n_ref + r) * d;
    const double c = sel_kern<KERN>(xr, xsc + ((size_t)k * n_cand + j) * d, d);
    double* __restrict__ H = isc ? V + (size_t)k * size * n_cand : Uh + (size_t)k * size * n_ref;
    const int ldh = isc ? n_cand : n_ref;
    const double* __restrict__ Vk = V + (size_t)k * size * n_cand;
    double hs = 0.0;
    for (int s = lane; s < t; s += 64) hs = fma(H[(size_t)s * ldh + r], Vk[(size_t)s * n_cand + j], hs);
    hs = wave_sum(hs);
    if (lane == 0) {
        const double den = fmax(h[(size_t)k * n_cand + j], 0.0) + 1.0 / (D * (double)nrep);
        H[(size_t)t * ldh + r] = (fma(-D, dot, coff * c) - hs) / sqrt(den);
    }
}

// (ii) y = U_ref^T (w o u), first half: ypart[k, chunk, col] over the SEL_RB reference rows of the chunk, one 16-byte piece of
// every row per thread
template <typename T>
__global__ __launch_bounds__(256) void sel_ty_part_kernel(const T* __restrict__ Ur, size_t sUr, int npad, int n, int n_ref,
                                                          const double* __restrict__ w, const double* __restrict__ Uh, int size,
                                                          int t, int nchunk, double* __restrict__ ypart) {
    constexpr int VN = SelVec<T>::N;
    typedef typename SelVec<T>::v V;
    __shared__ double wu[SEL_RB];
    const int ch = blockIdx.y, k = blockIdx.z, r0 = ch * SEL_RB;
    const int rows = min(SEL_RB, n_ref - r0);
    if (threadIdx.x < SEL_RB)
        wu[threadIdx.x] = threadIdx.x < rows ? w[r0 + threadIdx.x] * Uh[((size_t)k * size + t) * n_ref + r0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int col = (blockIdx.x * 256 + threadIdx.x) * VN;
    if (col >= n) return;
    const T* __restrict__ base = Ur + (size_t)k * sUr + (size_t)r0 * npad + col;
    double acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.0;
    // (columns n .. npad of a row belong to the slab: a whole piece is always readable; only columns < n are written)
#pragma unroll 8
    for (int i = 0; i < rows; ++i) {
        const V x = *(const V*)(base + (size_t)i * npad);
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[e] = fma((double)x[e], wu[i], acc[e]);
    }
    double* out = ypart + ((size_t)k * nchunk + ch) * npad + col;
#pragma unroll
    for (int e = 0; e < VN; ++e)
        if (col + e < n) out[e] = acc[e];
}

// second half: y[k, col] = sum of the chunks' partials in ascending order
__global__ __launch_bounds__(256) void sel_ty_reduce_kernel(const double* __restrict__ ypart, int nchunk, int npad, int n,
                                                            double* __restrict__ y) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (col >= npad) return;
    double s = 0.0;
    if (col < n) {
        const double* p = ypart + (size_t)k * nchunk * npad + col;
        for (int ch = 0; ch < nchunk; ++ch) s += p[(size_t)ch * npad];
    }
    y[(size_t)k * npad + col] = s;
}

// b[k, s] = Uh[s, :] . (w o u) for s <= t (s = t: u . (w o u)); one workgroup per (s, k), fixed-order sums
__global__ __launch_bounds__(256) void sel_hdot_kernel(const double* __restrict__ w, const double* __restrict__ Uh, int size,
                                                       int n_ref, int t, double* __restrict__ b) {
    __shared__ double red[256];
    const int s = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const double* __restrict__ us = Uh + ((size_t)k * size + s) * n_ref;
    const double* __restrict__ ut = Uh + ((size_t)k * size + t) * n_ref;
    double acc = 0.0;
    for (int i = tid; i < n_ref; i += 256) acc = fma(us[i], w[i] * ut[i], acc);
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) b[(size_t)k * size + s] = red[0];
}

// (iii) g(c) = C^x(c, ref) (w o u) - D U_cand(c) . y - sum_{s<t} V[s, c] b_s, then the update of the state of candidate c:
//   N = R den;  N <- max(N - 2 v g + v^2 b_t, 0);  h <- h - v^2;  R <- N / den(h)          v = V[t, c]
// one wave per candidate; the wave that holds the pick marks it
template <typename T, int KERN>
__global__ __launch_bounds__(256) void sel_update_kernel(const T* __restrict__ Uc, size_t sUc, int npad, int n, int n_cand, int n_ref,
                                                         const double* __restrict__ xsc, const double* __restrict__ xsr, int d,
                                                         const double* __restrict__ theta, int tw, int nrep,
                                                         const double* __restrict__ w, const double* __restrict__ y,
                                                         const double* __restrict__ b, const double* __restrict__ V,
                                                         const double* __restrict__ Uh, double* __restrict__ h,
                                                         double* __restrict__ R, int size, int t, const int* __restrict__ pick,
                                                         int* __restrict__ mask) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), k = blockIdx.y;
    if (c >= n_cand) return;                                // (uniform per wave)
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double coff = scale * (1.0 - nug / (1.0 + nug));
    const double dot = sel_row_dot_y<T>(Uc + (size_t)k * sUc + (size_t)c * npad, y + (size_t)k * npad, n, lane);
    const double* xc = xsc + ((size_t)k * n_cand + c) * d;
    const double* __restrict__ ut = Uh + ((size_t)k * size + t) * n_ref;
    double g1 = 0.0;
    for (int i = lane; i < n_ref; i += 64)
        g1 = fma(sel_kern<KERN>(xc, xsr + ((size_t)k * n_ref + i) * d, d), w[i] * ut[i], g1);
    g1 = wave_sum(g1);
    const double* __restrict__ Vk = V + (size_t)k * size * n_cand;
    const double* __restrict__ bk = b + (size_t)k * size;
    double hs = 0.0;
    for (int s = lane; s < t; s += 64) hs = fma(Vk[(size_t)s * n_cand + c], bk[s], hs);
    hs = wave_sum(hs);
    if (lane == 0) {
        const double g = fma(-D, dot, coff * g1) - hs;
        const double v = Vk[(size_t)t * n_cand + c], tau = 1.0 / (D * (double)nrep);
        const size_t o = (size_t)k * n_cand + c;
        const double h0 = h[o];
        const double N0 = R[o] * (fmax(h0, 0.0) + tau);
        const double N1 = fmax(fma(v * v, bk[t], fma(-2.0 * v, g, N0)), 0.0);
        const double h1 = fma(-v, v, h0);
        h[o] = h1;
        R[o] = N1 / (fmax(h1, 0.0) + tau);
        if (k == 0 && c == *pick) mask[c] = 1;
    }
}

// out[c] = sum over the local components, ascending, of omega_k R_k(c) (rounded products, rounded sums: what a host loop
// computes), -inf at picked candidates; then the argmax (lowest index wins ties) into *pick.  One workgroup.
__global__ __launch_bounds__(1024) void sel_score_kernel(const double* __restrict__ R, int q, int n_cand,
                                                         const double* __restrict__ omega, const int* __restrict__ mask,
                                                         double* __restrict__ out, int* __restrict__ pick) {
    __shared__ double bv[1024];
    __shared__ int bi[1024];
    const int tid = threadIdx.x;
    double best = -INFINITY;
    int at = 0x7fffffff;
    for (int c = tid; c < n_cand; c += 1024) {
        double s = -INFINITY;
        if (!mask[c]) {
            // (no contraction into fma: the product is rounded before it is added, as on the host)
#pragma clang fp contract(off)
            s = 0.0;
            for (int k = 0; k < q; ++k) {
                const double pr = omega[k] * R[(size_t)k * n_cand + c];
                s = s + pr;
            }
        }
        if (out) out[c] = s;
        if (s > best || at == 0x7fffffff) { best = s; at = c; }       // (ascending c: the first maximum stays)
    }
    bv[tid] = best; bi[tid] = at;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if (tid < o) {
            const double v2 = bv[tid + o];
            const int i2 = bi[tid + o];
            if (i2 != 0x7fffffff && (bi[tid] == 0x7fffffff || v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid]))) {
                bv[tid] = v2; bi[tid] = i2;
            }
        }
        __syncthreads();
    }
    if (tid == 0 && pick) *pick = bi[0];
}

template <typename T>
int do_sel_begin(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n_ref, const void* x_ref,
                 const double* w_ref, int n_cand, const void* x_cand, const int* match, int r, int size, int pass_rows,
                 char* scratch, const VrView* cv = nullptr) {
    const SelLay L = sel_carve(w.esz == 8 ? LCGP_F64 : LCGP_F32, w.n, w.d, w.q, n_ref, n_cand, size, cv ? cv->mpad : 0);
    const int tw = w.d + 3 + w.p;
    T* X = (T*)(scratch + L.off_x);
    T* ST = (T*)(scratch + L.off_st);
    T* Ur = (T*)(scratch + L.off_uref);
    T* Uc = (T*)(scratch + L.off_uc);
    double* hc = (double*)(scratch + L.off_h);
    int rc = vr_form<T>(st, w, x, sr, theta, n_ref, x_ref, nullptr, X, L.xslab, Ur, L.uslab_r, (double*)(scratch + L.off_ghr),
                        (double*)(scratch + L.off_gvr), n_ref, cv, ST);
    if (rc) return rc;
    for (int lo = 0; lo < n_cand; lo += pass_rows) {
        const int m = min(pass_rows, n_cand - lo);
        rc = vr_form<T>(st, w, x, sr, theta, m, (const T*)x_cand + (size_t)lo * w.d, match ? match + lo : nullptr, X, L.xslab,
                        Uc + (size_t)lo * L.kp, L.uslab_c, (double*)(scratch + L.off_ghc) + lo, hc + lo, n_cand, cv, ST);
        if (rc) return rc;
    }
    GemmArgs h;
    h.A = Ur; h.B = Uc; h.C = scratch + L.off_part;
    h.sA = L.uslab_r; h.sB = L.uslab_c; h.sC = 0;
    h.ldA = h.ldB = L.kp; h.ldC = 0;
    h.nb = 0;
    h.p0 = L.kp / TS; h.p1 = (n_cand + TS - 1) / TS; h.p2 = n_ref; h.p3 = n_cand;
    h.theta = theta; h.xa = x_ref; h.xb = x_cand; h.wref = w_ref; h.gvc = hc; h.ldg = n_cand;
    h.d = w.d; h.kern = w.kern; h.tw = tw; h.nrep = r; h.ldp = L.ldp;
    rc = launch_gemm<T, OP_VR, 64>(st, h, L.nrt * h.p1, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL(vr_reduce_kernel, dim3((n_cand + 255) / 256, w.q), dim3(256), 0, st, (const double*)(scratch + L.off_part),
                       L.nrt, L.ldp, n_cand, n_cand, (double*)(scratch + L.off_R));
    CHECK_LAUNCH("vr_reduce_kernel");
    hipLaunchKernelGGL((sel_scale_kernel<T>), dim3((n_ref * w.d + 255) / 256, w.q), dim3(256), 0, st, (const T*)x_ref, n_ref, w.d,
                       theta, tw, (double*)(scratch + L.off_xsr));
    CHECK_LAUNCH("sel_scale_kernel");
    hipLaunchKernelGGL((sel_scale_kernel<T>), dim3((n_cand * w.d + 255) / 256, w.q), dim3(256), 0, st, (const T*)x_cand, n_cand,
                       w.d, theta, tw, (double*)(scratch + L.off_xsc));
    CHECK_LAUNCH("sel_scale_kernel");
    const int mx = max(max(n_ref, n_cand), size);
    hipLaunchKernelGGL(sel_init_kernel, dim3((mx + 255) / 256), dim3(256), 0, st, w_ref, n_ref, (double*)(scratch + L.off_w), n_cand,
                       (int*)(scratch + L.off_mask), size, (int*)(scratch + L.off_picks));
    CHECK_LAUNCH("sel_init_kernel");
    return 0;
}

// one conditioning step on the pick *pick for all local components (w: n, d, p, q, kern, esz; no workspace is read).
// The row kernels take the row length ld and the length of the dot products kn: npad and n on the fitted model; on a
// conditioned view (mpad > 0) both are npad + mpad, the widened rows (zeros in their two paddings).
template <typename T>
int do_sel_condition(hipStream_t st, const Ws& w, const double* theta, int n_ref, int n_cand, int size, int r, int t,
                     const int* pick, char* scratch, int mpad = 0) {
    const SelLay L = sel_carve(w.esz == 8 ? LCGP_F64 : LCGP_F32, w.n, w.d, w.q, n_ref, n_cand, size, mpad);
    constexpr int VN = SelVec<T>::N;
    const int tw = w.d + 3 + w.p, ld = L.kp, kn = mpad ? L.kp : w.n;
    const T* Ur = (const T*)(scratch + L.off_uref);
    const T* Uc = (const T*)(scratch + L.off_uc);
    double* h = (double*)(scratch + L.off_h);
    double* R = (double*)(scratch + L.off_R);
    double* V = (double*)(scratch + L.off_V);
    double* Uh = (double*)(scratch + L.off_Uh);
    double* yp = (double*)(scratch + L.off_ypart);
    double* y = (double*)(scratch + L.off_y);
    double* b = (double*)(scratch + L.off_b);
    const double* xsr = (const double*)(scratch + L.off_xsr);
    const double* xsc = (const double*)(scratch + L.off_xsc);
    const double* wr = (const double*)(scratch + L.off_w);
    int* mask = (int*)(scratch + L.off_mask);
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((sel_col_kernel<T, decltype(kern)::value>), dim3((n_cand + n_ref + 3) / 4, w.q), dim3(256), 0, st, Uc,
                           L.uslab_c, Ur, L.uslab_r, ld, kn, n_cand, n_ref, xsc, xsr, w.d, theta, tw, r, (const double*)h, V, Uh,
                           size, t, pick);
    });
    CHECK_LAUNCH("sel_col_kernel");
    hipLaunchKernelGGL((sel_ty_part_kernel<T>), dim3((kn + 256 * VN - 1) / (256 * VN), L.nchunk, w.q), dim3(256), 0, st, Ur,
                       L.uslab_r, ld, kn, n_ref, wr, (const double*)Uh, size, t, L.nchunk, yp);
    CHECK_LAUNCH("sel_ty_part_kernel");
    hipLaunchKernelGGL(sel_ty_reduce_kernel, dim3((ld + 255) / 256, w.q), dim3(256), 0, st, (const double*)yp, L.nchunk, ld,
                       kn, y);
    CHECK_LAUNCH("sel_ty_reduce_kernel");
    hipLaunchKernelGGL(sel_hdot_kernel, dim3(t + 1, w.q), dim3(256), 0, st, wr, (const double*)Uh, size, n_ref, t, b);
    CHECK_LAUNCH("sel_hdot_kernel");
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((sel_update_kernel<T, decltype(kern)::value>), dim3((n_cand + 3) / 4, w.q), dim3(256), 0, st, Uc,
                           L.uslab_c, ld, kn, n_cand, n_ref, xsc, xsr, w.d, theta, tw, r, wr, (const double*)y, (const double*)b,
                           (const double*)V, (const double*)Uh, h, R, size, t, pick, mask);
    });
    CHECK_LAUNCH("sel_update_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// K8: input Hessians of the prediction.  For local component k, new input i (standardised) and dimensions m <= l, with
// s_l = (x0_il - x_jl) / ell_l, h = -(d/ds) log f and psi = f'' / f of the 1-D factor f (kern_h / kern_psi):
//   kap_lm(i, j) = h(s_l) h(s_m)  (l != m),   psi(s_l)  (l == m)              d2c_lm = c0 kap_lm / (ell_l ell_m)
//   d2ghat[k, i, lm] =         sum_j c0 kap_lm sr_j z_k[j]                  / (ell_l ell_m)
//   d2gvar[k, i, lm] = -2 D_k (sum_j c0 kap_lm sr_j V_k[i, j] + G_i[l, m]) / (ell_l ell_m)
//   G_i[l, m] = P[i d + l] . P[i d + m],   P = DX W^T,   DX[i d + l, j] = c0(i, j) sr_j h(s_l)     (the 1 / ell and the two signs
//   of d c0 / d x0_l = -c0 h / ell_l leave the rows and meet in the last step)
// Launches behind do_predict_grad: pdx_kernel (DX), OP_PRED_U of the tile kernel (P), phess_gram_kernel (G, into d2gvar),
// phess_kernel (the fused contraction, which reads G back and finishes both outputs).  The dimension pairs are worked in
// PH_B x PH_B blocks (lb >= mb) selected by blockIdx.z, so the accumulators per lane do not grow with d.  Fixed summation
// order, no atomics.
// ---------------------------------------------------------------------------------------------------
constexpr int PH_B = 4;        // dimensions per block of a block pair
constexpr int PH_PTS = 16;     // new inputs per workgroup of pdx_kernel

template <int KERN>
__device__ __forceinline__ double kern_h(double s) {
    if constexpr (KERN == 0) return s * fast_rcp(1.0 + fabs(s));
    else if constexpr (KERN == 1) return s;
    else {
        static_assert(KERN == 2, "unknown covariance kernel id");
        const double sa = fabs(s);
        return fma(s, sa, s) * fast_rcp(fma(sa, sa + 3.0, 3.0));
    }
}

template <int KERN>
__device__ __forceinline__ double kern_psi(double s) {
    const double sa = fabs(s);
    if constexpr (KERN == 0) return (sa - 1.0) * fast_rcp(1.0 + sa);
    else if constexpr (KERN == 1) return fma(s, s, -1.0);
    else {
        static_assert(KERN == 2, "unknown covariance kernel id");
        return fma(sa, sa - 1.0, -1.0) * fast_rcp(fma(sa, sa + 3.0, 3.0));
    }
}

template <int KERN>
__device__ __forceinline__ void kern_acc(double df, double& poly, double& ssum) {
    if constexpr (KERN == 0) {
        const double sd = fabs(df);
        poly *= 1.0 + sd;
        ssum -= sd;
    } else if constexpr (KERN == 1) {
        ssum = fma(-0.5 * df, df, ssum);
    } else {
        static_assert(KERN == 2, "unknown covariance kernel id");
        const double sd = fabs(df);
        poly = fma(poly, m52_fm1(sd), poly);
        ssum -= sd;
    }
}

// DX[k][i d + l, j] = c0(i, j) sr_j h(s_l) for i < n0, j < n; zero in the columns n .. npad and the rows n0 d .. rows_pad.
// One workgroup per (64 columns, PH_PTS new inputs, component): lane & 63 = column, each wave four inputs; c0 over all d
// in chunks of DMAX dimensions through LDS as cross_kernel forms it, then the d rows of each input (64 consecutive elements
// per wave and row).
template <typename T, int KERN>
__global__ __launch_bounds__(256) void pdx_kernel(T* __restrict__ DX, size_t slab, int ld, int n0, int n, int d, int rows_pad,
                                                  const T* __restrict__ x0, const T* __restrict__ x, const T* __restrict__ sr,
                                                  const double* __restrict__ theta, int tw) {
    __shared__ double xr[PH_PTS][DMAX + 1];
    __shared__ double xc[TS][DMAX + 1];
    __shared__ double cs[TS];
    __shared__ double th[DWIDE + 2];
    const int c = blockIdx.x, i0 = blockIdx.y * PH_PTS, k = blockIdx.z;
    const int tid = threadIdx.x, j = tid & 63, wv = tid >> 6, gj = c * TS + j;
    T* out = DX + (size_t)k * slab;
    for (int e = tid; e < d + 2; e += 256) th[e] = theta[(size_t)k * tw + e];
    if (tid < TS) cs[tid] = gj < n ? (sr ? (double)sr[gj] : 1.0) : 0.0;
    __syncthreads();
    const double scale = th[d], nug = th[d + 1];
    const double c_off = scale * (1.0 - nug / (1.0 + nug));
    auto stage = [&](int d0, int dc) {
        for (int e = tid; e < TS * dc; e += 256) {
            const int jj = e / dc, m = e - jj * dc, gjj = c * TS + jj;
            xc[jj][m] = gjj < n ? (double)x[(size_t)gjj * d + d0 + m] / th[d0 + m] : 0.0;
        }
        for (int e = tid; e < PH_PTS * dc; e += 256) {
            const int ii = e / dc, m = e - ii * dc;
            xr[ii][m] = i0 + ii < n0 ? (double)x0[(size_t)(i0 + ii) * d + d0 + m] / th[d0 + m] : 0.0;
        }
    };
    double poly[4], ssum[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { poly[a] = 1.0; ssum[a] = 0.0; }
    for (int d0 = 0; d0 < d; d0 += DMAX) {
        const int dc = d - d0 < DMAX ? d - d0 : DMAX;
        if (d0 > 0) __syncthreads();
        stage(d0, dc);
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a)
            for (int m = 0; m < dc; ++m) kern_acc<KERN>(xr[wv * 4 + a][m] - xc[j][m], poly[a], ssum[a]);
    }
    double v[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) v[a] = c_off * kern_c0<KERN>(poly[a], ssum[a]) * cs[j];      // (zero in the columns beyond n)
    const bool incol = gj < n;                           // (beyond n: +0, not v h = -0 where h < 0)
    for (int d0 = 0; d0 < d; d0 += DMAX) {
        const int dc = d - d0 < DMAX ? d - d0 : DMAX;
        if (d > DMAX) {                                  // (a single chunk is still resident)
            __syncthreads();
            stage(d0, dc);
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + wv * 4 + a;
            if (i >= n0) continue;
            T* row = out + ((size_t)i * d + d0) * ld + gj;
            for (int m = 0; m < dc; ++m)
                row[(size_t)m * ld] = incol ? (T)(v[a] * kern_h<KERN>(xr[wv * 4 + a][m] - xc[j][m])) : (T)0;
        }
    }
    if (blockIdx.y == gridDim.y - 1)
        for (int r = n0 * d + wv; r < rows_pad; r += 4) out[(size_t)r * ld + gj] = (T)0;
}

// G_i[l, m] = P[i d + l] . P[i d + m] over the n columns for the block pair blockIdx.z = (lb, mb), into the packed lower
// triangle of d2gvar (entries with m <= l < d).  One wave per new input: 16-byte loads of the 2 PH_B rows, PH_B^2
// accumulators in double, the fixed butterfly of wave_sum.
template <typename T>
__global__ __launch_bounds__(256) void phess_gram_kernel(const T* __restrict__ P, size_t slab, int ld, int n, int n0, int d,
                                                         int ldo, double* __restrict__ d2gvar) {
    constexpr int VN = SelVec<T>::N;
    typedef typename SelVec<T>::v V;
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), k = blockIdx.y;
    if (i >= n0) return;
    int lb, mb;
    tri_decode(blockIdx.z, lb, mb);
    const int l0 = lb * PH_B, m0 = mb * PH_B;
    const T* base = P + (size_t)k * slab + (size_t)i * d * ld;
    const T* ra[PH_B];
    const T* rb[PH_B];
#pragma unroll
    for (int a = 0; a < PH_B; ++a) {                    // (dimensions beyond d: row d - 1 again, never written out)
        ra[a] = base + (size_t)min(l0 + a, d - 1) * ld;
        rb[a] = base + (size_t)min(m0 + a, d - 1) * ld;
    }
    double acc[PH_B][PH_B];
#pragma unroll
    for (int a = 0; a < PH_B; ++a)
#pragma unroll
        for (int b = 0; b < PH_B; ++b) acc[a][b] = 0.0;
    const int nv = n / VN;
    for (int p = lane; p < nv; p += 64) {
        V xa[PH_B], xb[PH_B];
#pragma unroll
        for (int a = 0; a < PH_B; ++a) {
            xa[a] = *(const V*)(ra[a] + (size_t)p * VN);
            xb[a] = *(const V*)(rb[a] + (size_t)p * VN);
        }
#pragma unroll
        for (int a = 0; a < PH_B; ++a)
#pragma unroll
            for (int b = 0; b < PH_B; ++b)
#pragma unroll
                for (int e = 0; e < VN; ++e) acc[a][b] = fma((double)xa[a][e], (double)xb[b][e], acc[a][b]);
    }
    const int tail = nv * VN + lane;
    if (tail < n) {
#pragma unroll
        for (int a = 0; a < PH_B; ++a)
#pragma unroll
            for (int b = 0; b < PH_B; ++b) acc[a][b] = fma((double)ra[a][tail], (double)rb[b][tail], acc[a][b]);
    }
    double* o = d2gvar + ((size_t)k * ldo + i) * ((size_t)d * (d + 1) / 2);
#pragma unroll
    for (int a = 0; a < PH_B; ++a)
#pragma unroll
        for (int b = 0; b < PH_B; ++b) {
            const double s = wave_sum(acc[a][b]);
            const int l = l0 + a, m = m0 + b;
            if (lane == 0 && l < d && m <= l) o[l * (l + 1) / 2 + m] = s;
        }
}

// The fused second-derivative contraction, modelled on pgrad_kernel: one workgroup per (32 rows of x0, component, block
// pair): lane & 31 = row, the 8 half-waves take every 8th training input of a stage of JT.  c0 over all d from LDS, kap for
// the PH_B x PH_B entries of the block pair (2 PH_B^2 accumulators per lane whatever d), V staged through LDS; the n0 x n x
// d x d tensor is never written.  Per lane in ascending j, then the 8 slices in a fixed order.  The last step adds the Gram
// term phess_gram_kernel left in d2gvar and applies -2 D_k / (ell_l ell_m).  WIDE: d > 16 (rows of DWIDE + 3 doubles in LDS).
// COND (lcgp_condition_predict_hess): a SECOND segment of stages over the m conditioning inputs xn of a view behind the n
// training inputs, as in pgrad_body -- weight 1 instead of sr_j, w in place of z, R (rows mpad long) in place of V; z is the
// view's z' in double, and D rides on the weights of the first segment, so the last step applies -2 / (ell_l ell_m) to
// tv + D G.  Same stages, same lane / slice / wave order; per lane the training inputs in ascending j, then the conditioning
// inputs in ascending j.
template <typename T, int KERN, bool WIDE, bool COND>
__device__ __forceinline__ void phess_body(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                           const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                           int tw, const T* __restrict__ z, int npad, const T* __restrict__ V,
                                           size_t slab, int ldo, double* __restrict__ d2ghat,
                                           double* __restrict__ d2gvar, const PgradCond<T>& cs) {
    constexpr int JT = WIDE ? 16 : 32;                  // training inputs per LDS stage
    constexpr int XW = WIDE ? DWIDE + 3 : 16 + PH_B + 1; // odd row length >= l0 + PH_B for every block (zeros beyond d)
    __shared__ double x0sh[PG_ROWS][XW];
    __shared__ double xsh[JT][XW];
    __shared__ double vsh[PG_ROWS][JT + 1];
    __shared__ double wz[JT], wsr[JT];
    __shared__ double th[DWIDE + 3];
    __shared__ double red[2][4][PG_ROWS];
    const int k = blockIdx.y, i0 = blockIdx.x * PG_ROWS;
    int lb, mb;
    tri_decode(blockIdx.z, lb, mb);
    const int l0 = lb * PH_B, m0 = mb * PH_B;
    const bool diag = lb == mb;
    const int tid = threadIdx.x, r = tid & 31, sl = tid >> 5;
    for (int e = tid; e < d + 3; e += 256) th[e] = theta[(size_t)k * tw + e];
    __syncthreads();
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double c_off = scale * (1.0 - nug / (1.0 + nug));
    for (int e = tid; e < PG_ROWS * XW; e += 256) {
        const int i = e / XW, m = e - i * XW;
        x0sh[i][m] = (i0 + i < n0 && m < d) ? (double)x0[(size_t)(i0 + i) * d + m] / th[m] : 0.0;
    }
    const T* zk = COND ? z : z + (size_t)k * npad;       // (COND: z' comes in double through cs.zd)
    const T* Vk = V + (size_t)k * slab;
    double am[PH_B][PH_B], av[PH_B][PH_B];
#pragma unroll
    for (int a = 0; a < PH_B; ++a)
#pragma unroll
        for (int b = 0; b < PH_B; ++b) { am[a][b] = 0.0; av[a][b] = 0.0; }
    // (COND: the stages of the second segment follow those of the first, whose last stage may be short)
    const int n1 = (n + JT - 1) / JT * JT, jend = COND ? n1 + (cs.m + JT - 1) / JT * JT : n;
    for (int j0 = 0; j0 < jend; j0 += JT) {
        __syncthreads();                                // x0sh is written; every slice is done with the previous stage
        if constexpr (COND) {
            const bool seg2 = j0 >= n1;
            const int jb = seg2 ? j0 - n1 : j0;         // first input of the stage within its segment
            const T* xs = seg2 ? cs.xn : x;
            const int ns = seg2 ? cs.m : n;
            for (int e = tid; e < JT * XW; e += 256) {
                const int jj = e / XW, m = e - jj * XW;
                xsh[jj][m] = (jb + jj < ns && m < d) ? (double)xs[(size_t)(jb + jj) * d + m] / th[m] : 0.0;
            }
            for (int e = tid; e < PG_ROWS * JT; e += 256) {
                const int i = e / JT, jj = e - i * JT;
                const bool in = i0 + i < n0 && jb + jj < ns;
                vsh[i][jj] = !in ? 0.0 : seg2 ? (double)cs.R[(size_t)k * cs.rslab + (size_t)(i0 + i) * cs.mpad + jb + jj]
                                              : (double)Vk[(size_t)(i0 + i) * npad + jb + jj];
            }
            if (tid < JT) {
                const int j = jb + tid;
                const double s = j < ns ? (seg2 ? 1.0 : (sr ? (double)sr[j] : 1.0)) : 0.0;
                wsr[tid] = seg2 ? s : s * D;
                wz[tid] = j < ns ? s * (seg2 ? cs.wv[(size_t)k * cs.mpad + j] : cs.zd[(size_t)k * npad + j]) : 0.0;
            }
        } else {
            for (int e = tid; e < JT * XW; e += 256) {
                const int jj = e / XW, m = e - jj * XW;
                xsh[jj][m] = (j0 + jj < n && m < d) ? (double)x[(size_t)(j0 + jj) * d + m] / th[m] : 0.0;
            }
            for (int e = tid; e < PG_ROWS * JT; e += 256) {
                const int i = e / JT, jj = e - i * JT;
                vsh[i][jj] = (i0 + i < n0 && j0 + jj < n) ? (double)Vk[(size_t)(i0 + i) * npad + j0 + jj] : 0.0;
            }
            if (tid < JT) {
                const int j = j0 + tid;
                const double s = j < n ? (sr ? (double)sr[j] : 1.0) : 0.0;      // (inputs beyond n weigh zero)
                wsr[tid] = s;
                wz[tid] = j < n ? s * (double)zk[j] : 0.0;
            }
        }
        __syncthreads();
        for (int jj = sl; jj < JT; jj += PG_SL) {
            double poly = 1.0, ssum = 0.0;
            for (int m = 0; m < d; ++m) kern_acc<KERN>(x0sh[r][m] - xsh[jj][m], poly, ssum);
            const double c0 = c_off * kern_c0<KERN>(poly, ssum);
            const double ca = c0 * wz[jj], cb = c0 * wsr[jj] * vsh[r][jj];
            double hl[PH_B], hm[PH_B];
#pragma unroll
            for (int a = 0; a < PH_B; ++a) {
                hl[a] = kern_h<KERN>(x0sh[r][l0 + a] - xsh[jj][l0 + a]);
                hm[a] = kern_h<KERN>(x0sh[r][m0 + a] - xsh[jj][m0 + a]);
            }
#pragma unroll
            for (int a = 0; a < PH_B; ++a)
#pragma unroll
                for (int b = 0; b < PH_B; ++b) {
                    double kap = hl[a] * hm[b];
                    if (a == b && diag) kap = kern_psi<KERN>(x0sh[r][l0 + a] - xsh[jj][l0 + a]);
                    am[a][b] = fma(ca, kap, am[a][b]);
                    av[a][b] = fma(cb, kap, av[a][b]);
                }
        }
    }
    // slices 2w and 2w + 1 share wave w (lanes r, r + 32), then the four waves through LDS: a fixed order
    const int wave = tid >> 6, i = i0 + r;
    const size_t orow = ((size_t)k * ldo + i) * ((size_t)d * (d + 1) / 2);
#pragma unroll
    for (int a = 0; a < PH_B; ++a)
#pragma unroll
        for (int b = 0; b < PH_B; ++b) {
            const double sm = am[a][b] + __shfl_xor(am[a][b], 32), sv = av[a][b] + __shfl_xor(av[a][b], 32);
            if ((tid & 63) < 32) { red[0][wave][r] = sm; red[1][wave][r] = sv; }
            __syncthreads();
            const int l = l0 + a, m = m0 + b;
            if (tid < PG_ROWS && i < n0 && l < d && m <= l) {
                const double tm = (red[0][0][r] + red[0][1][r]) + (red[0][2][r] + red[0][3][r]);
                const double tv = (red[1][0][r] + red[1][1][r]) + (red[1][2][r] + red[1][3][r]);
                const double inv = 1.0 / (th[l] * th[m]);
                const size_t o = orow + (size_t)(l * (l + 1) / 2 + m);
                d2ghat[o] = tm * inv;
                if constexpr (COND) d2gvar[o] = -2.0 * (tv + D * d2gvar[o]) * inv;      // (D rode on the first segment's weights)
                else d2gvar[o] = -2.0 * D * (tv + d2gvar[o]) * inv;
            }
            __syncthreads();
        }
}

template <typename T, int KERN, bool WIDE>
__global__ __launch_bounds__(256) void phess_kernel(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                                    const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                                    int tw, const T* __restrict__ z, int npad, const T* __restrict__ V,
                                                    size_t slab, int ldo, double* __restrict__ d2ghat,
                                                    double* __restrict__ d2gvar) {
    phess_body<T, KERN, WIDE, false>(x0, n0, x, sr, n, d, theta, tw, z, npad, V, slab, ldo, d2ghat, d2gvar, PgradCond<T>{});
}

// the second-derivative contraction of lcgp_condition_predict_hess over the n training inputs and the m conditioning inputs
template <typename T, int KERN, bool WIDE>
__global__ __launch_bounds__(256) void phess_cond_kernel(const T* __restrict__ x0, int n0, const T* __restrict__ x,
                                                         const T* __restrict__ sr, int n, int d, const double* __restrict__ theta,
                                                         int tw, int npad, const T* __restrict__ V, size_t slab, int ldo,
                                                         double* __restrict__ d2ghat, double* __restrict__ d2gvar,
                                                         PgradCond<T> cs) {
    phess_body<T, KERN, WIDE, true>(x0, n0, x, sr, n, d, theta, tw, (const T*)nullptr, npad, V, slab, ldo, d2ghat, d2gvar, cs);
}

inline int hess_rows_pad(int n0, int d) { return predict_pad(n0 * d); }

// K8 for all local components: do_predict_grad (its four outputs bitwise those of lcgp_predict_grad; V_k stays in the X
// slab), then DX and P = DX W^T in the second half of the scratch, the Gram terms and the fused contraction.
template <typename T>
int do_predict_hess(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n0, const void* x0,
                    void* scratch, double* ghat, double* gvar, double* dghat, double* dgvar, double* d2ghat, double* d2gvar,
                    int ldo) {
    int rc = do_predict_grad<T>(st, w, x, sr, theta, n0, x0, scratch, ghat, gvar, dghat, dgvar, ldo);
    if (rc) return rc;
    const int n0pad = predict_pad(n0), rows_pad = hess_rows_pad(n0, w.d), tw = w.d + 3 + w.p;
    const size_t slab = (size_t)n0pad * w.npad, dslab = (size_t)rows_pad * w.npad;
    const T* V = (const T*)scratch;                     // q slabs n0pad x npad : X A^-1 (do_predict_grad)
    T* DX = (T*)scratch + 2 * slab * w.q;               // q slabs rows_pad x npad : c0 sr h(s_l), row i d + l
    T* P = DX + dslab * w.q;                            // q slabs rows_pad x npad : DX W^T
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((pdx_kernel<T, decltype(kern)::value>), dim3(w.nb, (n0 + PH_PTS - 1) / PH_PTS, w.q), dim3(256), 0, st,
                           DX, dslab, w.npad, n0, w.n, w.d, rows_pad, (const T*)x0, (const T*)x, (const T*)sr, theta, tw);
    });
    CHECK_LAUNCH("pdx_kernel");
    rc = launch_pred<T, OP_PRED_U>(st, DX, (const T*)(w.base + w.off_W), P, dslab, w.mat, w.npad, rows_pad, w.nb, w.q);
    if (rc) return rc;
    const int nblk = (w.d + PH_B - 1) / PH_B, npair = nblk * (nblk + 1) / 2;
    hipLaunchKernelGGL((phess_gram_kernel<T>), dim3((n0 + 3) / 4, w.q, npair), dim3(256), 0, st, (const T*)P, dslab, w.npad, w.n,
                       n0, w.d, ldo, d2gvar);
    CHECK_LAUNCH("phess_gram_kernel");
    dim3 grid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, npair);
    for_kern(w.kern, [&](auto kern) {
        auto go = [&](auto wide) {
            hipLaunchKernelGGL((phess_kernel<T, decltype(kern)::value, decltype(wide)::value>), grid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, w.n, w.d, theta, tw, (const T*)(w.base + w.off_z),
                               w.npad, V, slab, ldo, d2ghat, d2gvar);
        };
        if (w.d > 16) go(std::true_type{});
        else go(std::false_type{});
    });
    CHECK_LAUNCH("phess_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// K9: posterior covariance of the latent gradient (lcgp_hip.h: lcgp_predict_gradcov).  For local component k,
// new input i and dimensions m <= l, with the rows P of K8 (their factors -1 / ell left out):
//   Gamma[k, i, lm] = (delta_lm c_k kappa - D_k P[i d + l] . P[i d + m]) / (ell_l ell_m),   c_k = scale (1 - nug / (1 + nug))
//   M[k, lm]       += sum_i w_i Gamma[k, i, lm]
// Launches: pgrad_kernel<MEAN> (dghat, bitwise that of K7), pdx_kernel, OP_PRED_U of the tile kernel, gradcov_kernel, and with
// weights gradcov_reduce_kernel.  V_k = U_k W_k and the contractions over the training inputs of K8 are not needed.
// ---------------------------------------------------------------------------------------------------

// phess_gram_kernel's dot products for the block pair blockIdx.z, finished to Gamma: one wave per new input, the packed
// lower triangle to `gamma` unless it is NULL.  With weights the four waves' w_i Gamma go through LDS and are summed in wave
// order into part[k][blockIdx.x][lm]: every entry of the triangle by exactly one block pair.
template <typename T>
__global__ __launch_bounds__(256) void gradcov_kernel(const T* __restrict__ P, size_t slab, int ld, int n, int n0, int d,
                                                      const double* __restrict__ theta, int tw, double kappa, int ldo,
                                                      double* __restrict__ gamma, const double* __restrict__ w,
                                                      double* __restrict__ part) {
    constexpr int VN = SelVec<T>::N;
    typedef typename SelVec<T>::v V;
    __shared__ double red[4][PH_B * PH_B];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i = blockIdx.x * 4 + wv, k = blockIdx.y;
    const bool live = i < n0;                           // (uniform over the wave)
    int lb, mb;
    tri_decode(blockIdx.z, lb, mb);
    const int l0 = lb * PH_B, m0 = mb * PH_B;
    const size_t tri = (size_t)d * (d + 1) / 2;
    const double* th = theta + (size_t)k * tw;
    double acc[PH_B][PH_B];
#pragma unroll
    for (int a = 0; a < PH_B; ++a)
#pragma unroll
        for (int b = 0; b < PH_B; ++b) acc[a][b] = 0.0;
    if (live) {
        const T* base = P + (size_t)k * slab + (size_t)i * d * ld;
        const T* ra[PH_B];
        const T* rb[PH_B];
#pragma unroll
        for (int a = 0; a < PH_B; ++a) {                // (dimensions beyond d: row d - 1 again, never written out)
            ra[a] = base + (size_t)min(l0 + a, d - 1) * ld;
            rb[a] = base + (size_t)min(m0 + a, d - 1) * ld;
        }
        const int nv = n / VN;
        for (int p = lane; p < nv; p += 64) {
            V xa[PH_B], xb[PH_B];
#pragma unroll
            for (int a = 0; a < PH_B; ++a) {
                xa[a] = *(const V*)(ra[a] + (size_t)p * VN);
                xb[a] = *(const V*)(rb[a] + (size_t)p * VN);
            }
#pragma unroll
            for (int a = 0; a < PH_B; ++a)
#pragma unroll
                for (int b = 0; b < PH_B; ++b)
#pragma unroll
                    for (int e = 0; e < VN; ++e) acc[a][b] = fma((double)xa[a][e], (double)xb[b][e], acc[a][b]);
        }
        const int tail = nv * VN + lane;
        if (tail < n) {
#pragma unroll
            for (int a = 0; a < PH_B; ++a)
#pragma unroll
                for (int b = 0; b < PH_B; ++b) acc[a][b] = fma((double)ra[a][tail], (double)rb[b][tail], acc[a][b]);
        }
    }
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double prior = scale * (1.0 - nug / (1.0 + nug)) * kappa;
    const double wi = (w && live) ? w[i] : 0.0;
    double* o = gamma ? gamma + ((size_t)k * ldo + (live ? i : 0)) * tri : nullptr;
#pragma unroll
    for (int a = 0; a < PH_B; ++a)
#pragma unroll
        for (int b = 0; b < PH_B; ++b) {
            const double s = wave_sum(acc[a][b]);
            const int l = l0 + a, m = m0 + b;
            double g = 0.0;
            if (live && l < d && m <= l) {
                g = ((l == m ? prior : 0.0) - D * s) / (th[l] * th[m]);
                if (lane == 0 && o) o[l * (l + 1) / 2 + m] = g;
            }
            if (lane == 0) red[wv][a * PH_B + b] = wi * g;
        }
    if (!w) return;                                     // (uniform over the launch)
    __syncthreads();
    const int t = threadIdx.x;
    if (t < PH_B * PH_B) {
        const int l = l0 + t / PH_B, m = m0 + t % PH_B;
        if (l < d && m <= l)
            part[((size_t)k * gridDim.x + blockIdx.x) * tri + (size_t)(l * (l + 1) / 2 + m)] =
                ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

// M[k][e] += the nwg partial sums of gradcov_kernel in ascending workgroup order
__global__ __launch_bounds__(256) void gradcov_reduce_kernel(const double* __restrict__ part, int nwg, int tri,
                                                             double* __restrict__ M) {
    const int e = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (e >= tri) return;
    const double* p = part + (size_t)k * nwg * tri + e;
    double s = 0.0;
    for (int g = 0; g < nwg; ++g) s += p[(size_t)g * tri];
    M[(size_t)k * tri + e] += s;
}

inline double gradcov_kappa(int kern) { return kern == LCGP_KERNEL_MATERN52 ? 1.0 / 3.0 : 1.0; }

// K9 for all local components.  Scratch: DX and P (q slabs rows_pad x npad each); once P is formed the DX slabs are free
// and take the per-workgroup partial sums (q ceil(n0 / 4) tri doubles <= 508 q n0 d bytes < q rows_pad npad elements).
template <typename T>
int do_predict_gradcov(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int n0, const void* x0,
                       void* scratch, double* dghat, double* gamma, const double* wt, double* M, int ldo) {
    const int rows_pad = hess_rows_pad(n0, w.d), tw = w.d + 3 + w.p;
    const size_t dslab = (size_t)rows_pad * w.npad;
    T* DX = (T*)scratch;
    T* P = DX + dslab * w.q;
    const int wide = w.d > 16;
    dim3 pgrid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, wide ? (w.d + DMAX - 1) / DMAX : 1);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((pgrad_kernel<T, decltype(dd)::value, decltype(kern)::value, false, true>), pgrid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, w.n, w.d, theta, tw, (const T*)(w.base + w.off_z),
                               w.npad, (const T*)nullptr, (size_t)0, ldo, dghat, (double*)nullptr);
        });
    });
    CHECK_LAUNCH("pgrad_kernel");
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((pdx_kernel<T, decltype(kern)::value>), dim3(w.nb, (n0 + PH_PTS - 1) / PH_PTS, w.q), dim3(256), 0, st,
                           DX, dslab, w.npad, n0, w.n, w.d, rows_pad, (const T*)x0, (const T*)x, (const T*)sr, theta, tw);
    });
    CHECK_LAUNCH("pdx_kernel");
    int rc = launch_pred<T, OP_PRED_U>(st, DX, (const T*)(w.base + w.off_W), P, dslab, w.mat, w.npad, rows_pad, w.nb, w.q);
    if (rc) return rc;
    const int nblk = (w.d + PH_B - 1) / PH_B, npair = nblk * (nblk + 1) / 2, nwg = (n0 + 3) / 4, tri = w.d * (w.d + 1) / 2;
    double* part = (double*)scratch;
    hipLaunchKernelGGL((gradcov_kernel<T>), dim3(nwg, w.q, npair), dim3(256), 0, st, (const T*)P, dslab, w.npad, w.n, n0, w.d,
                       theta, tw, gradcov_kappa(w.kern), ldo, gamma, wt, part);
    CHECK_LAUNCH("gradcov_kernel");
    if (wt) {
        hipLaunchKernelGGL(gradcov_reduce_kernel, dim3((tri + 255) / 256, w.q), dim3(256), 0, st, (const double*)part, nwg, tri, M);
        CHECK_LAUNCH("gradcov_reduce_kernel");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// K8 / K9 on a conditioned view (lcgp_hip.h: lcgp_condition_predict_hess / lcgp_condition_predict_gradcov).  The
// derivative rows of K8 are formed on both column sets and widened to K' = npad + mpad as the rows of the design criteria
// are (vr_form):
//   P_il  = DX_il W^T                                            (npad; pdx_kernel on (x0, x, sr), OP_PRED_U)
//   Q_il  = (DX^n_il - D P_il U_n^T) L_S^-T                        (mpad; pdx_kernel on (x0, xn, no sr), OP_COND_CROSS, OP_PRED_U
//                                                                 on the dense L_S^-1: the launches that make T out of X_0)
//   P'_il = [ P_il | Q_il / sqrt(D) ]                            (cond_rows_tail_kernel: zeros in the columns m .. mpad - 1)
// so that D P'_il . P'_im is the Gram term of the augmented factor; the columns n .. npad - 1 of P are zero, and the unchanged
// Gram kernels sum npad + m columns of rows K' apart.
//   d2ghat'[i, lm] =     (sum_j c0 kap sr_j z'_j      + sum_a c0^x kap w_a)                       / (ell_l ell_m)
//   d2gvar'[i, lm] = -2 (D sum_j c0 kap sr_j V'[i, j] + sum_a c0^x kap R[i, a] + D P'_il . P'_im) / (ell_l ell_m)
//   Gamma'[i, lm]  = (delta_lm c_k kappa - D P'_il . P'_im) / (ell_l ell_m)
// ---------------------------------------------------------------------------------------------------

// out[r, 0 .. mpad) = Q[r, :] / sqrt(D_k) behind column npad of the widened row r (ldu apart) for r < rows; zeros in the columns
// m .. mpad - 1 and in the rows rows .. gridDim.x - 1, whatever the scratch held: cond_tail_kernel without the gvar update
template <typename T>
__global__ __launch_bounds__(64) void cond_rows_tail_kernel(const T* __restrict__ Q, size_t slab, int m, int mpad, int rows,
                                                            const double* __restrict__ theta, int tw, int d, T* __restrict__ Pt,
                                                            size_t pslab, int ldu) {
    const int r = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    T* out = Pt + (size_t)k * pslab + (size_t)r * ldu;
    if (r >= rows) {                                // (uniform per block)
        for (int j = lane; j < mpad; j += 64) out[j] = (T)0;
        return;
    }
    const T* Qr = Q + (size_t)k * slab + (size_t)r * mpad;
    const double is = 1.0 / sqrt(theta[(size_t)k * tw + d + 2]);
    for (int j = lane; j < mpad; j += 64) out[j] = j < m ? (T)((double)Qr[j] * is) : (T)0;
}

// scratch of the widened derivative rows of one pass: P' (q slabs rows_pad x K'), DX (q rows_pad x npad), DX^n and Q (q rows_pad x
// mpad each) = q rows_pad (2 K' + mpad) elements, carved in this order by cond_rows_form
inline size_t cond_rows_scratch(int dtype, int n, int d, int q, int m, int n0) {
    const size_t mpad = cov_pad(m), kp = (size_t)round_up(n, 2 * TS) + mpad;
    return align256((size_t)q * hess_rows_pad(n0, d) * (2 * kp + mpad) * (dtype == LCGP_F64 ? 8 : 4));
}

// P' for all local components into Pw (q slabs rows_pad x K'); DX, DX^n and Q behind it
template <typename T>
int cond_rows_form(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const T* Un, const T* Wi, int m,
                   int mpad, const void* xn, int n0, const void* x0, T* Pw) {
    const int rows_pad = hess_rows_pad(n0, w.d), tw = w.d + 3 + w.p, kp = w.npad + mpad;
    const size_t pslab = (size_t)rows_pad * kp, dslab = (size_t)rows_pad * w.npad, cslab = (size_t)rows_pad * mpad;
    T* DX = Pw + pslab * w.q;
    T* Sd = DX + dslab * w.q;
    T* Qm = Sd + cslab * w.q;
    // (the carve above against the size the entries check the caller's scratch with: a mismatch is an error, not a fault)
    if ((size_t)(Qm + cslab * w.q - Pw) * sizeof(T) > cond_rows_scratch(sizeof(T) == 4 ? LCGP_F32 : LCGP_F64, w.n, w.d, w.q, m, n0))
        return bad("internal: the widened derivative rows do not fit lcgp_condition_predict_gradcov_scratch_bytes");
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((pdx_kernel<T, decltype(kern)::value>), dim3(w.nb, (n0 + PH_PTS - 1) / PH_PTS, w.q), dim3(256), 0, st,
                           DX, dslab, w.npad, n0, w.n, w.d, rows_pad, (const T*)x0, (const T*)x, (const T*)sr, theta, tw);
    });
    CHECK_LAUNCH("pdx_kernel");
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((pdx_kernel<T, decltype(kern)::value>), dim3(mpad / TS, (n0 + PH_PTS - 1) / PH_PTS, w.q), dim3(256), 0, st,
                           Sd, cslab, mpad, n0, m, w.d, rows_pad, (const T*)x0, (const T*)xn, (const T*)nullptr, theta, tw);
    });
    CHECK_LAUNCH("pdx_kernel (view inputs)");
    int rc = launch_pred<T, OP_PRED_U>(st, DX, (const T*)(w.base + w.off_W), Pw, dslab, w.mat, w.npad, rows_pad, w.nb, w.q, pslab,
                                       false, kp);
    if (rc) return rc;
    GemmArgs h;
    h.A = Pw; h.B = Un; h.C = Sd;
    h.sA = pslab; h.sB = (size_t)mpad * w.npad; h.sC = cslab; h.ldA = kp; h.ldB = w.npad; h.ldC = mpad;
    h.nb = 0; h.p0 = w.npad / TS; h.p1 = mpad / TS; h.p2 = tw; h.p3 = w.d + 2;
    h.theta = theta;
    rc = launch_gemm<T, OP_COND_CROSS, 64>(st, h, (rows_pad / TS) * (mpad / TS), w.q);
    if (rc) return rc;
    rc = launch_pred<T, OP_PRED_U>(st, Sd, Wi, Qm, cslab, (size_t)mpad * mpad, mpad, rows_pad, mpad / TS, w.q);
    if (rc) return rc;
    hipLaunchKernelGGL((cond_rows_tail_kernel<T>), dim3(rows_pad, w.q), dim3(64), 0, st, (const T*)Qm, cslab, m, mpad, n0 * w.d, theta,
                       tw, w.d, Pw + w.npad, pslab, kp);
    CHECK_LAUNCH("cond_rows_tail_kernel");
    return 0;
}

// K8 on a view: do_condition_predict_grad (its four outputs bitwise those of lcgp_condition_predict_grad; V' stays in the X slab,
// R over Sigma_0n), then the widened rows behind that pass's scratch, the Gram terms and the two-segment contraction.
template <typename T>
int do_condition_predict_hess(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const void* state,
                              int m, const void* xn, const void* gstate, int n0, const void* x0, void* scratch, double* ghat,
                              double* gvar, double* dghat, double* dgvar, double* d2ghat, double* d2gvar, int ldo) {
    int rc = do_condition_predict_grad<T>(st, w, x, sr, theta, state, m, xn, gstate, n0, x0, scratch, ghat, gvar, dghat, dgvar, ldo);
    if (rc) return rc;
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const CondLay L = cond_carve(dtype, w.n, w.q, m);
    const CondGradLay G = cond_grad_carve(w.n, w.q, m);
    const int mpad = L.mpad, n0pad = predict_pad(n0), rows_pad = hess_rows_pad(n0, w.d), tw = w.d + 3 + w.p, kp = w.npad + mpad;
    const size_t slab = (size_t)n0pad * w.npad, cslab = (size_t)n0pad * mpad;
    const T* Un = (const T*)((const char*)state + L.off_U);
    const T* Wi = (const T*)((const char*)state + L.off_W);
    const T* V = (const T*)scratch;                     // V' = U' W (do_condition_predict_grad)
    const T* Rm = (const T*)((const char*)scratch + align256(2 * (size_t)w.q * slab * sizeof(T)));
    T* Pw = (T*)((char*)scratch + cond_predict_scratch(dtype, w.n, w.q, m, n0));
    rc = cond_rows_form<T>(st, w, x, sr, theta, Un, Wi, m, mpad, xn, n0, x0, Pw);
    if (rc) return rc;
    const int nblk = (w.d + PH_B - 1) / PH_B, npair = nblk * (nblk + 1) / 2;
    hipLaunchKernelGGL((phess_gram_kernel<T>), dim3((n0 + 3) / 4, w.q, npair), dim3(256), 0, st, (const T*)Pw,
                       (size_t)rows_pad * kp, kp, w.npad + m, n0, w.d, ldo, d2gvar);
    CHECK_LAUNCH("phess_gram_kernel");
    PgradCond<T> cs;
    cs.zd = (const double*)((const char*)gstate + G.off_z);
    cs.xn = (const T*)xn; cs.m = m;
    cs.wv = (const double*)((const char*)gstate + G.off_w); cs.mpad = mpad;
    cs.R = Rm; cs.rslab = cslab;
    dim3 grid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, npair);
    for_kern(w.kern, [&](auto kern) {
        auto go = [&](auto wide) {
            hipLaunchKernelGGL((phess_cond_kernel<T, decltype(kern)::value, decltype(wide)::value>), grid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, w.n, w.d, theta, tw, w.npad, V, slab, ldo, d2ghat,
                               d2gvar, cs);
        };
        if (w.d > 16) go(std::true_type{});
        else go(std::false_type{});
    });
    CHECK_LAUNCH("phess_cond_kernel");
    return 0;
}

// K9 on a view.  Scratch: cond_rows_scratch; once P is formed the DX slabs are free and take the per-workgroup partial sums
// exactly as in do_predict_gradcov (the same q ceil(n0 / 4) tri doubles in the same q rows_pad npad elements: they still fit).
template <typename T>
int do_condition_predict_gradcov(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, const void* state,
                                 int m, const void* xn, const void* gstate, int n0, const void* x0, void* scratch, double* dghat,
                                 double* gamma, const double* wt, double* M, int ldo) {
    const int dtype = sizeof(T) == 4 ? LCGP_F32 : LCGP_F64;
    const CondLay L = cond_carve(dtype, w.n, w.q, m);
    const CondGradLay G = cond_grad_carve(w.n, w.q, m);
    const int mpad = L.mpad, rows_pad = hess_rows_pad(n0, w.d), tw = w.d + 3 + w.p, kp = w.npad + mpad;
    const T* Un = (const T*)((const char*)state + L.off_U);
    const T* Wi = (const T*)((const char*)state + L.off_W);
    PgradCond<T> cs;
    cs.zd = (const double*)((const char*)gstate + G.off_z);
    cs.xn = (const T*)xn; cs.m = m;
    cs.wv = (const double*)((const char*)gstate + G.off_w); cs.mpad = mpad;
    cs.R = nullptr; cs.rslab = 0;
    const int wide = w.d > 16;
    dim3 pgrid((n0 + PG_ROWS - 1) / PG_ROWS, w.q, wide ? (w.d + DMAX - 1) / DMAX : 1);
    for_dim(w.d, [&](auto dd) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((pgrad_cond_mean_kernel<T, decltype(dd)::value, decltype(kern)::value>), pgrid, dim3(256), 0, st,
                               (const T*)x0, n0, (const T*)x, (const T*)sr, w.n, w.d, theta, tw, w.npad, ldo, dghat, cs);
        });
    });
    CHECK_LAUNCH("pgrad_cond_mean_kernel");
    T* Pw = (T*)scratch;
    int rc = cond_rows_form<T>(st, w, x, sr, theta, Un, Wi, m, mpad, xn, n0, x0, Pw);
    if (rc) return rc;
    const size_t pslab = (size_t)rows_pad * kp;
    const int nblk = (w.d + PH_B - 1) / PH_B, npair = nblk * (nblk + 1) / 2, nwg = (n0 + 3) / 4, tri = w.d * (w.d + 1) / 2;
    double* part = (double*)(Pw + pslab * w.q);         // the DX slabs
    hipLaunchKernelGGL((gradcov_kernel<T>), dim3(nwg, w.q, npair), dim3(256), 0, st, (const T*)Pw, pslab, kp, w.npad + m, n0, w.d,
                       theta, tw, gradcov_kappa(w.kern), ldo, gamma, wt, part);
    CHECK_LAUNCH("gradcov_kernel");
    if (wt) {
        hipLaunchKernelGGL(gradcov_reduce_kernel, dim3((tri + 255) / 256, w.q), dim3(256), 0, st, (const double*)part, nwg, tri, M);
        CHECK_LAUNCH("gradcov_reduce_kernel");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Hessian of the objective in the parameters (lcgp_hip.h: lcgp_nll_hess; no counterpart in the reference, whose
// users would nest two gradient tapes around neglpost).  float64 only.  Runs behind lcgp_nll_grad at the same theta and only
// READS the workspace (A^-1 lower tiles, b, z).  Per component, m = d + 2 kernel parameters [ell_0 .. ell_{d-1}, scale, nug]:
//   AI = A^-1 mirrored to a full matrix; G_scale, G_nug elementwise from it (d_scale A and d_nug A are combinations of A, I and
//   diag(s^2));  for every dimension i: E = d_iA materialised (one buffer, reused), y_i = E z, G_i = AI E on the tile kernel
//   (OP_HESS_G);  tr(G_i G_j) by a tile-transposing reduction;  sum gmat o d_ijC by a fused contraction that recomputes C0,
//   phi_i and d phi_i / d ell_i in registers;  u_i = AI y_i, Q = Y AI (tile kernel), and the small dot products.
// Every sum has a fixed order (per-thread ascending, butterflies, per-band partials summed ascending), no atomics: bitwise
// reproducible, independent of the number of components in the call and of the scratch content on entry.
// ---------------------------------------------------------------------------------------------------
constexpr int HS_B = 4;            // dimensions per block of a block pair of the second-order contraction
constexpr int HS_SLOTS = 22;       // 16 second-order sums, 4 first-order sums, sum gmat o C0, trace gmat
constexpr int HS_JC = 8;           // G_j tiles multiplied against one staged G_i tile

struct HessLay {
    int m, npad, nb, ppad, npair, nbk, npb;
    size_t mat;
    size_t off_ai, off_e, off_g, off_xs, off_yv, off_uv, off_yp, off_q, off_tp, off_cp, off_dot, total;
};

inline HessLay hess_carve(int n, int d, int p, int qg) {
    HessLay H;
    H.m = d + 2;
    H.npad = round_up(n, 2 * TS);
    H.nb = H.npad / TS;
    H.ppad = round_up(p, 2 * TS);
    H.npair = H.m * (H.m + 1) / 2;
    H.nbk = (d + HS_B - 1) / HS_B;
    H.npb = H.nbk * (H.nbk + 1) / 2;
    H.mat = (size_t)H.npad * H.npad;
    size_t o = 0;
    const size_t e = sizeof(double);
    H.off_ai = o; o = align256(o + (size_t)qg * H.mat * e);
    H.off_e = o; o = align256(o + (size_t)qg * H.mat * e);
    H.off_g = o; o = align256(o + (size_t)qg * H.m * H.mat * e);
    H.off_xs = o; o = align256(o + (size_t)qg * d * H.npad * e);
    H.off_yv = o; o = align256(o + (size_t)qg * H.m * H.npad * e);
    H.off_uv = o; o = align256(o + (size_t)qg * H.m * H.npad * e);
    H.off_yp = o; o = align256(o + (size_t)H.ppad * H.npad * e);
    H.off_q = o; o = align256(o + (size_t)qg * H.ppad * H.npad * e);
    H.off_tp = o; o = align256(o + (size_t)qg * H.npair * H.nb * e);
    H.off_cp = o; o = align256(o + (size_t)qg * H.npb * H.nb * HS_SLOTS * e);
    H.off_dot = o; o = align256(o + (size_t)qg * H.m * H.m * e);
    H.total = o;
    return H;
}

inline int hess_out_width(int d, int p) { return (d + 2) * (d + 2) + (d + 2) * p + p * p; }

// phi = d log C0 / d ell and d phi / d ell of one dimension at S = |dx| / ell
template <int KERN>
__device__ __forceinline__ void hess_phi(double S, double ell, double& phi, double& dphi) {
    static_assert(kern_known<KERN>::value, "unknown covariance kernel id");
    const double ie = 1.0 / ell, S2 = S * S;
    if constexpr (KERN == 0) {
        const double r = 1.0 / (1.0 + S);
        phi = S2 * r * ie;
        dphi = -S2 * fma(2.0, S, 3.0) * (r * r) * (ie * ie);
    } else if constexpr (KERN == 1) {
        phi = S2 * ie;
        dphi = -3.0 * S2 * (ie * ie);
    } else {
        const double r = 1.0 / fma(S, S, fma(3.0, S, 3.0));
        const double N = S2 * (1.0 + S);
        phi = N * r * ie;
        dphi = -(S2 * fma(3.0, S, 2.0) * r + N * (3.0 - S2) * (r * r)) * (ie * ie);
    }
}

// C0(a, b) from the inputs divided by ell, stored dimension-major (xs[l * npad + i])
template <int KERN>
__device__ __forceinline__ double hess_c0(const double* __restrict__ xs, int npad, int d, int a, int b) {
    double poly = 1.0, ssum = 0.0;
    for (int l = 0; l < d; ++l) {
        const double df = xs[(size_t)l * npad + a] - xs[(size_t)l * npad + b];
        if constexpr (KERN == 0) {
            const double sd = fabs(df);
            poly = fma(poly, sd, poly);
            ssum -= sd;
        } else if constexpr (KERN == 1) {
            ssum = fma(-0.5 * df, df, ssum);
        } else {
            static_assert(KERN == 2, "unknown covariance kernel id");
            const double sd = fabs(df);
            poly = fma(poly, m52_fm1(sd), poly);
            ssum -= sd;
        }
    }
    return kern_c0<KERN>(poly, ssum);
}

// sum over the 256 threads of a workgroup in a fixed order (butterflies inside a wave, then the four waves); sh: 4 doubles
__device__ __forceinline__ double hess_block_sum(double v, double* sh, int tid) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// xs = x / ell (dimension-major, zero beyond n) and the two vectors that need no matrix: y_scale = d_scale A z = (b - z) / scale,
// y_nug = d_nug A z = [D scale s^2 o z - (b - z)] / ((1 - w) (1 + nug)^2)        (A z = b)
__global__ __launch_bounds__(256) void hess_prep_kernel(const double* __restrict__ x, const double* __restrict__ sr, int n, int npad,
                                                        int d, const double* __restrict__ theta, int tw,
                                                        const double* __restrict__ bvec, const double* __restrict__ zvec,
                                                        double* __restrict__ xs, double* __restrict__ yv) {
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i >= npad) return;
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    double* xk = xs + (size_t)k * d * npad;
    for (int l = 0; l < d; ++l) xk[(size_t)l * npad + i] = i < n ? x[(size_t)i * d + l] / th[l] : 0.0;
    double* yk = yv + (size_t)k * (d + 2) * npad;
    double ys = 0.0, yn = 0.0;
    if (i < n) {
        const double z = zvec[(size_t)k * npad + i], bz = bvec[(size_t)k * npad + i] - z;
        const double s = sr ? sr[i] : 1.0;
        ys = bz / scale;
        yn = (D * scale * (s * s) * z - bz) / (1.0 + nug);      // 1 / ((1 - w) (1 + nug)^2) = 1 / (1 + nug)
    }
    yk[(size_t)d * npad + i] = ys;
    yk[(size_t)(d + 1) * npad + i] = yn;
}

// AI = A^-1 as a full symmetric matrix (identity on the padding) from the lower tiles of the workspace, and beside it
//   G_scale = A^-1 d_scale A = (I - A^-1) / scale,     G_nug = A^-1 d_nug A = [D scale A^-1 diag(s^2) - I + A^-1] / (1 + nug)
// (zero on the padding)
__global__ __launch_bounds__(256) void hess_mirror_kernel(const double* __restrict__ V, size_t mat, int n, int npad, int d,
                                                          const double* __restrict__ sr, const double* __restrict__ theta, int tw,
                                                          double* __restrict__ AI, double* __restrict__ G) {
    const int b = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y, k = blockIdx.z;
    if (b >= npad) return;
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const bool in = a < n && b < n;
    const double* Vk = V + (size_t)k * mat;
    const double dl = a == b ? 1.0 : 0.0;
    const double v = in ? (b <= a ? Vk[(size_t)a * npad + b] : Vk[(size_t)b * npad + a]) : dl;
    const size_t e = (size_t)a * npad + b;
    AI[(size_t)k * mat + e] = v;
    double* Gk = G + (size_t)k * (d + 2) * mat;
    const double sb = (sr && b < n) ? sr[b] : 1.0;
    Gk[(size_t)d * mat + e] = in ? (dl - v) / scale : 0.0;
    Gk[(size_t)(d + 1) * mat + e] = in ? (fma(D * scale * (sb * sb), v, v) - dl) / (1.0 + nug) : 0.0;
}

// E = d A / d ell_i = D scale (1 - w) (s s^T) o C0 o phi_i as a full matrix, zero on the padding
template <int KERN>
__global__ __launch_bounds__(256) void hess_da_kernel(double* __restrict__ E, size_t mat, int n, int npad, int d, int i,
                                                      const double* __restrict__ xs, const double* __restrict__ sr,
                                                      const double* __restrict__ theta, int tw) {
    const int b = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y, k = blockIdx.z;
    if (b >= npad) return;
    double v = 0.0;
    if (a < n && b < n) {
        const double* th = theta + (size_t)k * tw;
        const double scale = th[d], nug = th[d + 1], D = th[d + 2];
        const double* xk = xs + (size_t)k * d * npad;
        const double c0 = hess_c0<KERN>(xk, npad, d, a, b);
        double phi, dphi;
        hess_phi<KERN>(fabs(xk[(size_t)i * npad + a] - xk[(size_t)i * npad + b]), th[i], phi, dphi);
        const double ss = sr ? sr[a] * sr[b] : 1.0;
        v = (D * scale / (1.0 + nug)) * ss * c0 * phi;
    }
    E[(size_t)k * mat + (size_t)a * npad + b] = v;
}

// O[v][r] = sum_c M[r, c] X[v][c]: one wave per row, the lanes stride the columns, butterflies at the end
__global__ __launch_bounds__(256) void hess_matvec_kernel(const double* __restrict__ M, size_t sM, int n, int npad,
                                                          const double* __restrict__ X, size_t sXk, double* __restrict__ O, size_t sOk) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6), v = blockIdx.y, k = blockIdx.z;
    const double* row = M + (size_t)k * sM + (size_t)r * npad;
    const double* xv = X + (size_t)k * sXk + (size_t)v * npad;
    double s = 0.0;
    for (int c = lane; c < n; c += 64) s = fma(row[c], xv[c], s);      // (columns beyond n hold the padding: exact zeros in M)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) O[(size_t)k * sOk + (size_t)v * npad + r] = s;
}

// partial traces: tp[k][pair(i, j <= i)][rb] = sum_{a in band rb} sum_b G_i[a, b] G_j[b, a].  One workgroup per (band, i, chunk of
// HS_JC values of j): the 64 x 64 tile G_i[rb, tb] is staged in LDS and read transposed against the tiles G_j[tb, rb]
__global__ __launch_bounds__(256) void hess_trace_kernel(const double* __restrict__ G, size_t mat, int npad, int nb, int m, int npair,
                                                         double* __restrict__ tp) {
    __shared__ double T[TS][TS + 1];
    __shared__ double sh[4];
    const int njc = (m + HS_JC - 1) / HS_JC;
    const int rb = blockIdx.x, i = blockIdx.y / njc, j0 = (blockIdx.y % njc) * HS_JC, k = blockIdx.z;
    if (j0 > i) return;
    const int tid = threadIdx.x, c = tid & 63, r0 = tid >> 6;
    const double* Gk = G + (size_t)k * m * mat;
    const double* Gi = Gk + (size_t)i * mat;
    double acc[HS_JC];
#pragma unroll
    for (int jj = 0; jj < HS_JC; ++jj) acc[jj] = 0.0;
    for (int tb = 0; tb < nb; ++tb) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) T[r0 + 4 * e][c] = Gi[(size_t)(rb * TS + r0 + 4 * e) * npad + tb * TS + c];
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < HS_JC; ++jj) {
            if (j0 + jj <= i) {
                const double* Gj = Gk + (size_t)(j0 + jj) * mat + (size_t)(tb * TS) * npad + rb * TS + c;
                double s = acc[jj];
#pragma unroll
                for (int e = 0; e < 16; ++e) s = fma(Gj[(size_t)(r0 + 4 * e) * npad], T[c][r0 + 4 * e], s);
                acc[jj] = s;
            }
        }
    }
#pragma unroll
    for (int jj = 0; jj < HS_JC; ++jj) {
        if (j0 + jj <= i) {          // (uniform over the workgroup)
            const double s = hess_block_sum(acc[jj], sh, tid);
            if (tid == 0) tp[((size_t)k * npair + (size_t)i * (i + 1) / 2 + j0 + jj) * nb + rb] = s;
        }
    }
}

// The second-order fused contraction: with gmat = s s^T o (D/2 A^-1 - z z^T / 2) (the weight of the gradient contraction) and
// w0 = gmat o C0, for the band rb of 64 rows and the block pair (bi, bj <= bi) of HS_B dimensions each
//   slot ii * 4 + jj : sum w0 (phi_i phi_j + [i == j] d phi_i / d ell_i),   i = 4 bi + ii, j = 4 bj + jj
//   slot 16 + ii     : sum w0 phi_i        (bj == 0 only)
//   slot 20, 21      : sum w0, trace gmat  (block pair 0 only)
// C0, phi and d phi are recomputed in registers from the scaled inputs: no n x n x d x d tensor is written
template <int KERN>
__global__ __launch_bounds__(256) void hess_contract_kernel(const double* __restrict__ AI, size_t mat, int n, int npad, int nb, int d,
                                                            const double* __restrict__ xs, const double* __restrict__ sr,
                                                            const double* __restrict__ zvec, const double* __restrict__ theta, int tw,
                                                            int npb, double* __restrict__ cp) {
    __shared__ double sh[4];
    const int rb = blockIdx.x, pb = blockIdx.y, k = blockIdx.z;
    int bi, bj;
    tri_decode(pb, bi, bj);
    const int tid = threadIdx.x, cl = tid & 63, r0 = tid >> 6;
    const double* th = theta + (size_t)k * tw;
    const double D = th[d + 2];
    const double* xk = xs + (size_t)k * d * npad;
    const double* zk = zvec + (size_t)k * npad;
    const double* Ak = AI + (size_t)k * mat;
    double a2[HS_B][HS_B], a1[HS_B], a0 = 0.0, ad = 0.0;
#pragma unroll
    for (int ii = 0; ii < HS_B; ++ii) {
        a1[ii] = 0.0;
#pragma unroll
        for (int jj = 0; jj < HS_B; ++jj) a2[ii][jj] = 0.0;
    }
    for (int tb = 0; tb < nb; ++tb) {
        const int b = tb * TS + cl;
        if (b >= n) continue;
        const double zb = zk[b], sb = sr ? sr[b] : 1.0;
        for (int e = 0; e < 16; ++e) {
            const int a = rb * TS + r0 + 4 * e;
            if (a >= n) continue;
            const double sa = sr ? sr[a] : 1.0;
            const double g = (sa * sb) * (0.5 * D * Ak[(size_t)a * npad + b] - 0.5 * (zk[a] * zb));
            const double w0 = g * hess_c0<KERN>(xk, npad, d, a, b);
            a0 += w0;
            if (a == b) ad += g;
            double pi[HS_B], dpi[HS_B], pj[HS_B];
#pragma unroll
            for (int ii = 0; ii < HS_B; ++ii) {
                const int li = bi * HS_B + ii, lj = bj * HS_B + ii;
                pi[ii] = dpi[ii] = pj[ii] = 0.0;
                if (li < d) hess_phi<KERN>(fabs(xk[(size_t)li * npad + a] - xk[(size_t)li * npad + b]), th[li], pi[ii], dpi[ii]);
                if (bi == bj) pj[ii] = pi[ii];
                else if (lj < d) {
                    double unused;
                    hess_phi<KERN>(fabs(xk[(size_t)lj * npad + a] - xk[(size_t)lj * npad + b]), th[lj], pj[ii], unused);
                }
            }
#pragma unroll
            for (int ii = 0; ii < HS_B; ++ii) {
                a1[ii] = fma(w0, pi[ii], a1[ii]);
#pragma unroll
                for (int jj = 0; jj < HS_B; ++jj) {
                    const double k2 = (bi == bj && ii == jj) ? fma(pi[ii], pj[jj], dpi[ii]) : pi[ii] * pj[jj];
                    a2[ii][jj] = fma(w0, k2, a2[ii][jj]);
                }
            }
        }
    }
    double* out = cp + (((size_t)k * npb + pb) * nb + rb) * HS_SLOTS;
#pragma unroll
    for (int ii = 0; ii < HS_B; ++ii)
#pragma unroll
        for (int jj = 0; jj < HS_B; ++jj) {
            const double s = hess_block_sum(a2[ii][jj], sh, tid);
            if (tid == 0) out[ii * HS_B + jj] = s;
        }
#pragma unroll
    for (int ii = 0; ii < HS_B; ++ii) {
        const double s = hess_block_sum(a1[ii], sh, tid);
        if (tid == 0) out[16 + ii] = s;
    }
    const double s0 = hess_block_sum(a0, sh, tid), sd = hess_block_sum(ad, sh, tid);
    if (tid == 0) { out[20] = s0; out[21] = sd; }
}

// dot[k][i * m + j] = y_i . u_j  (u_j = A^-1 y_j): one wave per pair
__global__ __launch_bounds__(64) void hess_dot_kernel(const double* __restrict__ yv, const double* __restrict__ uv, int n, int npad, int m,
                                                      double* __restrict__ dot) {
    const int i = blockIdx.x / m, j = blockIdx.x % m, k = blockIdx.y, lane = threadIdx.x;
    const double* y = yv + ((size_t)k * m + i) * npad;
    const double* u = uv + ((size_t)k * m + j) * npad;
    double s = 0.0;
    for (int c = lane; c < n; c += 64) s = fma(y[c], u[c], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) dot[(size_t)k * m * m + blockIdx.x] = s;
}

// Y (p x n) zero padded to ppad x npad: the A operand of Q = Y A^-1
__global__ __launch_bounds__(256) void hess_pack_y_kernel(const double* __restrict__ Y, int p, int n, int npad, double* __restrict__ YP) {
    const int i = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
    if (i >= npad) return;
    YP[(size_t)a * npad + i] = (a < p && i < n) ? Y[(size_t)a * n + i] : 0.0;
}

// cross block: hx[i * p + a] = psi_a (Y_a . u_i) / (2 D): one wave per entry
__global__ __launch_bounds__(64) void hess_cross_kernel(const double* __restrict__ YP, const double* __restrict__ uv, int n, int npad, int m,
                                                        int p, int d, const double* __restrict__ theta, int tw, double* __restrict__ out,
                                                        int ow) {
    const int i = blockIdx.x / p, a = blockIdx.x % p, k = blockIdx.y, lane = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    const double* y = YP + (size_t)a * npad;
    const double* u = uv + ((size_t)k * m + i) * npad;
    double s = 0.0;
    for (int c = lane; c < n; c += 64) s = fma(y[c], u[c], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[(size_t)k * ow + m * m + blockIdx.x] = th[d + 3 + a] * s / (2.0 * th[d + 2]);
}

// noise block: hn[a * p + b] = -[ delta_ab psi_a Y_a . (b - z) + psi_a psi_b Y_a . (Y_b - Q_b) ] / (4 D),  Q_b = A^-1 Y_b
__global__ __launch_bounds__(64) void hess_noise_kernel(const double* __restrict__ YP, const double* __restrict__ Q, size_t sQ, int n, int npad,
                                                        int m, int p, int d, const double* __restrict__ bvec,
                                                        const double* __restrict__ zvec, const double* __restrict__ theta, int tw,
                                                        double* __restrict__ out, int ow) {
    const int a = blockIdx.x / p, b = blockIdx.x % p, k = blockIdx.y, lane = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    const double* ya = YP + (size_t)a * npad;
    const double* yb = YP + (size_t)b * npad;
    const double* qb = Q + (size_t)k * sQ + (size_t)b * npad;
    const double* bk = bvec + (size_t)k * npad;
    const double* zk = zvec + (size_t)k * npad;
    double s = 0.0, t = 0.0;
    for (int c = lane; c < n; c += 64) {
        s = fma(ya[c], yb[c] - qb[c], s);
        if (a == b) t = fma(ya[c], bk[c] - zk[c], t);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); t += __shfl_xor(t, o); }
    if (lane == 0) {
        const double pa = th[d + 3 + a], pb = th[d + 3 + b];
        out[(size_t)k * ow + m * m + m * p + blockIdx.x] = -(pa * t + pa * pb * s) / (4.0 * th[d + 2]);
    }
}

// kernel block: hk[i][j] = T_ij - tr(G_i G_j) / 2 + y_i . u_j / D, one thread per pair i >= j, written to both triangles.
// T_ij = sum gmat o d_ij C from the slots of hess_contract_kernel, the bands summed in ascending order
__global__ __launch_bounds__(256) void hess_final_kernel(const double* __restrict__ tp, const double* __restrict__ cp,
                                                         const double* __restrict__ dot, int nb, int m, int npair, int npb, int d,
                                                         const double* __restrict__ theta, int tw, double* __restrict__ out, int ow) {
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (t >= npair) return;
    int i, j;
    tri_decode(t, i, j);
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double w1 = 1.0 / ((1.0 + nug) * (1.0 + nug)), omw = 1.0 / (1.0 + nug);      // dw / dnug, 1 - w
    const double* cpk = cp + (size_t)k * npb * nb * HS_SLOTS;
    auto slot_sum = [&](int pb, int slot) {
        double s = 0.0;
        for (int rb = 0; rb < nb; ++rb) s += cpk[((size_t)pb * nb + rb) * HS_SLOTS + slot];
        return s;
    };
    double T;
    if (i < d) {                       // (j <= i < d)
        const int bi = i / HS_B, bj = j / HS_B;
        T = scale * omw * slot_sum(bi * (bi + 1) / 2 + bj, (i % HS_B) * HS_B + j % HS_B);
    } else if (j < d) {                // (scale | nug) x ell_j
        const int bj = j / HS_B;
        const double s1 = slot_sum(bj * (bj + 1) / 2, 16 + j % HS_B);
        T = i == d ? omw * s1 : -scale * w1 * s1;
    } else {
        const double dd = slot_sum(0, 21) - slot_sum(0, 20);       // sum gmat o (I - C0)
        T = (i == d) ? 0.0 : (j == d ? w1 * dd : -2.0 * scale * w1 * omw * dd);
    }
    double tr = 0.0;
    const double* tpk = tp + ((size_t)k * npair + t) * nb;
    for (int rb = 0; rb < nb; ++rb) tr += tpk[rb];
    const double v = (T - 0.5 * tr) + dot[(size_t)k * m * m + (size_t)i * m + j] / D;
    out[(size_t)k * ow + (size_t)i * m + j] = v;
    out[(size_t)k * ow + (size_t)j * m + i] = v;
}

// enqueues the pass for the components [k0, k0 + qg) of the workspace; `out` rows are those of the q_local components
int do_nll_hess(hipStream_t st, const Ws& w, const void* x, const double* Y, const void* sr, const double* theta, int k0, int qg,
                char* scratch, double* out) {
    const int n = w.n, d = w.d, p = w.p, npad = w.npad, tw = d + 3 + p, ow = hess_out_width(d, p);
    const HessLay H = hess_carve(n, d, p, qg);
    const int m = H.m, nb = H.nb;
    double* AI = (double*)(scratch + H.off_ai);
    double* E = (double*)(scratch + H.off_e);
    double* G = (double*)(scratch + H.off_g);
    double* XS = (double*)(scratch + H.off_xs);
    double* YV = (double*)(scratch + H.off_yv);
    double* UV = (double*)(scratch + H.off_uv);
    double* YP = (double*)(scratch + H.off_yp);
    double* Q = (double*)(scratch + H.off_q);
    double* TP = (double*)(scratch + H.off_tp);
    double* CP = (double*)(scratch + H.off_cp);
    double* DOT = (double*)(scratch + H.off_dot);
    const double* V = (const double*)(w.base + w.off_V) + (size_t)k0 * w.mat;
    const double* bv = (const double*)(w.base + w.off_b) + (size_t)k0 * npad;
    const double* zv = (const double*)(w.base + w.off_z) + (size_t)k0 * npad;
    const double* th = theta + (size_t)k0 * tw;
    const double* xd = (const double*)x;
    const double* srd = (const double*)sr;
    double* o = out + (size_t)k0 * ow;
    const dim3 full((npad + 255) / 256, npad, qg);

    hipLaunchKernelGGL(hess_prep_kernel, dim3((npad + 255) / 256, qg), dim3(256), 0, st, xd, srd, n, npad, d, th, tw, bv, zv, XS, YV);
    CHECK_LAUNCH("hess_prep_kernel");
    hipLaunchKernelGGL(hess_mirror_kernel, full, dim3(256), 0, st, V, w.mat, n, npad, d, srd, th, tw, AI, G);
    CHECK_LAUNCH("hess_mirror_kernel");
    GemmArgs g;
    g.A = AI; g.B = E; g.ldA = g.ldB = g.ldC = npad;
    g.sA = H.mat; g.sB = H.mat; g.sC = (size_t)m * H.mat;
    g.nb = nb / 2; g.p0 = nb / 2; g.p1 = nb / 2; g.p2 = g.p3 = 0;
    for (int i = 0; i < d; ++i) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((hess_da_kernel<decltype(kern)::value>), full, dim3(256), 0, st, E, H.mat, n, npad, d, i,
                               (const double*)XS, srd, th, tw);
        });
        CHECK_LAUNCH("hess_da_kernel");
        // y_i = d_iA z
        hipLaunchKernelGGL(hess_matvec_kernel, dim3(npad / 4, 1, qg), dim3(256), 0, st, (const double*)E, H.mat, n, npad, zv, (size_t)npad,
                           YV + (size_t)i * npad, (size_t)m * npad);
        CHECK_LAUNCH("hess_matvec_kernel");
        g.C = G + (size_t)i * H.mat;
        int rc = launch_gemm<double, OP_HESS_G, 128>(st, g, g.p0 * g.nb, qg);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(hess_trace_kernel, dim3(nb, m * ((m + HS_JC - 1) / HS_JC), qg), dim3(256), 0, st, (const double*)G, H.mat, npad,
                       nb, m, H.npair, TP);
    CHECK_LAUNCH("hess_trace_kernel");
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((hess_contract_kernel<decltype(kern)::value>), dim3(nb, H.npb, qg), dim3(256), 0, st, (const double*)AI, H.mat,
                           n, npad, nb, d, (const double*)XS, srd, zv, th, tw, H.npb, CP);
    });
    CHECK_LAUNCH("hess_contract_kernel");
    // u_i = A^-1 y_i for all m vectors
    hipLaunchKernelGGL(hess_matvec_kernel, dim3(npad / 4, m, qg), dim3(256), 0, st, (const double*)AI, H.mat, n, npad, (const double*)YV,
                       (size_t)m * npad, UV, (size_t)m * npad);
    CHECK_LAUNCH("hess_matvec_kernel");
    hipLaunchKernelGGL(hess_dot_kernel, dim3(m * m, qg), dim3(64), 0, st, (const double*)YV, (const double*)UV, n, npad, m, DOT);
    CHECK_LAUNCH("hess_dot_kernel");
    // Q = Y A^-1 (Y zero padded to whole tiles; A^-1 symmetric: row b of Q is A^-1 Y_b)
    hipLaunchKernelGGL(hess_pack_y_kernel, dim3((npad + 255) / 256, H.ppad), dim3(256), 0, st, Y, p, n, npad, YP);
    CHECK_LAUNCH("hess_pack_y_kernel");
    GemmArgs gq;
    gq.A = YP; gq.B = AI; gq.C = Q; gq.ldA = gq.ldB = gq.ldC = npad;
    gq.sA = 0; gq.sB = H.mat; gq.sC = (size_t)H.ppad * npad;
    gq.nb = nb / 2; gq.p0 = H.ppad / (2 * TS); gq.p1 = nb / 2; gq.p2 = gq.p3 = 0;
    int rc = launch_gemm<double, OP_HESS_G, 128>(st, gq, gq.p0 * gq.nb, qg);
    if (rc) return rc;
    hipLaunchKernelGGL(hess_cross_kernel, dim3(m * p, qg), dim3(64), 0, st, (const double*)YP, (const double*)UV, n, npad, m, p, d, th, tw,
                       o, ow);
    CHECK_LAUNCH("hess_cross_kernel");
    hipLaunchKernelGGL(hess_noise_kernel, dim3(p * p, qg), dim3(64), 0, st, (const double*)YP, (const double*)Q, (size_t)H.ppad * npad, n,
                       npad, m, p, d, bv, zv, th, tw, o, ow);
    CHECK_LAUNCH("hess_noise_kernel");
    hipLaunchKernelGGL(hess_final_kernel, dim3((H.npair + 255) / 256, qg), dim3(256), 0, st, (const double*)TP, (const double*)CP,
                       (const double*)DOT, nb, m, H.npair, H.npb, d, th, tw, o, ow);
    CHECK_LAUNCH("hess_final_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Parameter derivatives of the prediction (lcgp_hip.h: lcgp_predict_paramgrad; the reference would put a gradient
// tape around predict over the trainable variables).  float64 only.  Runs behind lcgp_nll_grad at the same theta and only
// READS the workspace (L^-1, b, z).  Per component and new input i, with X_i the cross-covariance row of lcgp_predict,
// V_i = X_i A^-1, y_t = d_tA z and the m = d + 2 kernel parameters t in [ell_0 .. ell_{d-1}, scale, nug]:
//     d_t ghat_i = (d_t X_i) . z - V_i . y_t          d_t gvar_i = d_t scale - D [2 (d_t X_i) . V_i - V_i (d_tA) V_i^T]
// Launches: hess_prep_kernel (x / ell, y_scale, y_nug); X, U = X W^T, ghat / gvar and V = U W exactly as lcgp_predict_grad forms
// them (V over X); per dimension j: d_jA materialised (hess_da_kernel, one buffer), y_j = d_jA z, T_j = V d_jA on the tile kernel
// (OP_HESS_G, over U) and its row dots with V; the fused row kernel (C0 and phi_j recomputed in registers, every other sum of
// the formulas in one sweep over the row); V Y^T on the tile kernel; the combining kernel.
// Every sum has a fixed order, no atomics: bitwise reproducible, independent of the number of components in the call and of
// the scratch content on entry.
// ---------------------------------------------------------------------------------------------------
constexpr int PP_DB = 16;          // dimensions per workgroup of the row kernel: 3 accumulators each, 48 of the 56 per thread

struct PgradLay {
    int m, npad, nb, ppad, n0p, n0r, nsum;
    size_t mat, slab;
    size_t off_x, off_u, off_e, off_xs, off_yv, off_yt, off_vy, off_rd, off_sum, total;
};

inline PgradLay pgrad_carve(int n, int d, int p, int qg, int n0) {
    PgradLay L;
    L.m = d + 2;
    L.npad = round_up(n, 2 * TS);
    L.nb = L.npad / TS;
    L.ppad = round_up(p, 2 * TS);
    L.n0p = predict_pad(n0);                // rows of X / U / V the launches of lcgp_predict form
    L.n0r = round_up(n0, 2 * TS);           // rows of a slab: the dense products run on 128 x 128 tiles
    L.nsum = 3 * d + 8;                     // [ dz_j (d) | dv_j (d) | Xc.z, Xc.V, rz, rv, |V|^2, sum s^2 V^2 | V . y_t (d + 2) ]
    L.mat = (size_t)L.npad * L.npad;
    L.slab = (size_t)L.n0r * L.npad;
    size_t o = 0;
    const size_t e = sizeof(double);
    L.off_x = o; o = align256(o + (size_t)qg * L.slab * e);
    L.off_u = o; o = align256(o + (size_t)qg * L.slab * e);
    L.off_e = o; o = align256(o + (size_t)qg * L.mat * e);
    L.off_xs = o; o = align256(o + (size_t)qg * d * L.npad * e);
    L.off_yv = o; o = align256(o + (size_t)qg * L.m * L.npad * e);
    L.off_yt = o; o = align256(o + (size_t)L.npad * L.ppad * e);
    L.off_vy = o; o = align256(o + (size_t)qg * L.n0r * L.ppad * e);
    L.off_rd = o; o = align256(o + (size_t)qg * d * L.n0r * e);
    L.off_sum = o; o = align256(o + (size_t)qg * L.n0r * L.nsum * e);
    L.total = o;
    return L;
}

// Y^T (n x p) zero padded to npad x ppad: the B operand of V Y^T
__global__ __launch_bounds__(256) void pgrad_pack_yt_kernel(const double* __restrict__ Y, int p, int n, int ppad, double* __restrict__ YT) {
    const int a = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (a >= ppad) return;
    YT[(size_t)i * ppad + a] = (a < p && i < n) ? Y[(size_t)a * n + i] : 0.0;
}

// rd[k][j][i] = T_j[i, :] . V[i, :] = V_i (d_jA) V_i^T: one wave per new input
__global__ __launch_bounds__(64) void pgrad_rowdot_kernel(const double* __restrict__ T, const double* __restrict__ V, size_t slab, int ld,
                                                          int n, double* __restrict__ rd, size_t srd) {
    const int i = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const double* t = T + (size_t)k * slab + (size_t)i * ld;
    const double* v = V + (size_t)k * slab + (size_t)i * ld;
    double s = 0.0;
    for (int c = lane; c < n; c += 64) s = fma(t[c], v[c], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) rd[(size_t)k * srd + i] = s;
}

// The fused row kernel: one workgroup per (new input i, component, block of PP_DB dimensions).  With Xc = scale (1 - w) C0 o s
// the continuous part of the cross-covariance row (C0 and phi_j recomputed in registers from x / ell), v = V_i and c* the
// column of the row's nugget entry (same > 0: c* = i + same - 1), one sweep over the n columns accumulates
//   dz_j = sum Xc phi_j z      dv_j = sum Xc phi_j v      vy_j = sum v y_j             for the block's dimensions j
//   Xc . z, Xc . v, rz = s z at c*, rv = s v at c*, |v|^2, sum s^2 v^2, v . y_scale, v . y_nug       (dimension block 0 only)
// into row (k, i) of `sums` (PgradLay::nsum doubles).  No n0 x n x d tensor is written.
template <int KERN>
__global__ __launch_bounds__(256) void pgrad_row_kernel(const double* __restrict__ x0, int n0, int same, const double* __restrict__ xs,
                                                        const double* __restrict__ sr, int n, int npad, int d,
                                                        const double* __restrict__ theta, int tw, const double* __restrict__ zvec,
                                                        const double* __restrict__ V, size_t slab, const double* __restrict__ yv,
                                                        double* __restrict__ sums, int n0r, int nsum) {
    __shared__ double x0l[DWIDE];
    __shared__ double sh[4];
    const int i = blockIdx.x, k = blockIdx.y, j0 = blockIdx.z * PP_DB, tid = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    if (tid < d) x0l[tid] = x0[(size_t)i * d + tid] / th[tid];
    __syncthreads();
    const double cc = th[d] / (1.0 + th[d + 1]);          // scale (1 - w)
    const double* xk = xs + (size_t)k * d * npad;
    const double* zk = zvec + (size_t)k * npad;
    const double* vr = V + (size_t)k * slab + (size_t)i * npad;
    const double* yk = yv + (size_t)k * (d + 2) * npad;
    const int cstar = same > 0 ? i + same - 1 : -1;
    const bool first = j0 == 0;
    double dz[PP_DB], dv[PP_DB], vy[PP_DB];
#pragma unroll
    for (int jj = 0; jj < PP_DB; ++jj) dz[jj] = dv[jj] = vy[jj] = 0.0;
    double xz = 0.0, xv = 0.0, rz = 0.0, rv = 0.0, vv = 0.0, s2vv = 0.0, vys = 0.0, vyn = 0.0;
    for (int c = tid; c < n; c += 256) {
        double poly = 1.0, ssum = 0.0;
        for (int l = 0; l < d; ++l) {
            const double df = x0l[l] - xk[(size_t)l * npad + c];
            if constexpr (KERN == 0) {
                const double sd = fabs(df);
                poly = fma(poly, sd, poly);
                ssum -= sd;
            } else if constexpr (KERN == 1) {
                ssum = fma(-0.5 * df, df, ssum);
            } else {
                static_assert(KERN == 2, "unknown covariance kernel id");
                const double sd = fabs(df);
                poly = fma(poly, m52_fm1(sd), poly);
                ssum -= sd;
            }
        }
        const double s = sr ? sr[c] : 1.0, z = zk[c], v = vr[c];
        const double xc = cc * kern_c0<KERN>(poly, ssum) * s;
#pragma unroll
        for (int jj = 0; jj < PP_DB; ++jj) {
            const int j = j0 + jj;
            if (j < d) {
                double phi, dphi;
                hess_phi<KERN>(fabs(x0l[j] - xk[(size_t)j * npad + c]), th[j], phi, dphi);
                const double t = xc * phi;
                dz[jj] = fma(t, z, dz[jj]);
                dv[jj] = fma(t, v, dv[jj]);
                vy[jj] = fma(v, yk[(size_t)j * npad + c], vy[jj]);
            }
        }
        if (first) {
            xz = fma(xc, z, xz);
            xv = fma(xc, v, xv);
            vv = fma(v, v, vv);
            s2vv = fma((s * s) * v, v, s2vv);
            vys = fma(v, yk[(size_t)d * npad + c], vys);
            vyn = fma(v, yk[(size_t)(d + 1) * npad + c], vyn);
            if (c == cstar) { rz = s * z; rv = s * v; }
        }
    }
    double* out = sums + ((size_t)k * n0r + i) * nsum;
#pragma unroll
    for (int jj = 0; jj < PP_DB; ++jj) {
        const int j = j0 + jj;
        if (j < d) {                 // (uniform over the workgroup)
            const double a = hess_block_sum(dz[jj], sh, tid), b = hess_block_sum(dv[jj], sh, tid), c = hess_block_sum(vy[jj], sh, tid);
            if (tid == 0) { out[j] = a; out[d + j] = b; out[2 * d + 6 + j] = c; }
        }
    }
    if (first) {
        const double a0 = hess_block_sum(xz, sh, tid), a1 = hess_block_sum(xv, sh, tid), a2 = hess_block_sum(rz, sh, tid),
                     a3 = hess_block_sum(rv, sh, tid), a4 = hess_block_sum(vv, sh, tid), a5 = hess_block_sum(s2vv, sh, tid),
                     a6 = hess_block_sum(vys, sh, tid), a7 = hess_block_sum(vyn, sh, tid);
        if (tid == 0) {
            double* o6 = out + 2 * d;
            o6[0] = a0; o6[1] = a1; o6[2] = a2; o6[3] = a3; o6[4] = a4; o6[5] = a5;
            out[3 * d + 6] = a6; out[3 * d + 7] = a7;
        }
    }
}

// combines the sums into dghat / dgvar (n0 x (d + 2), order [ell_0 .. ell_{d-1}, scale, nug]) and dghat_noise (n0 x p):
// one thread per (new input, component)
__global__ __launch_bounds__(256) void pgrad_final_kernel(const double* __restrict__ sums, int n0r, int nsum, const double* __restrict__ rd,
                                                          const double* __restrict__ vy, int ppad, int n0, int d, int p,
                                                          const double* __restrict__ theta, int tw, int ldo,
                                                          double* __restrict__ dghat, double* __restrict__ dgvar,
                                                          double* __restrict__ dnoise) {
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i >= n0) return;
    const double* th = theta + (size_t)k * tw;
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double omw = 1.0 / (1.0 + nug), nt = nug * omw, w1 = omw * omw;      // 1 - w, w, dw / dnug
    const double* s = sums + ((size_t)k * n0r + i) * nsum;
    const double* rdk = rd + (size_t)k * d * n0r;
    const int m = d + 2;
    double* dg = dghat + ((size_t)k * ldo + i) * m;
    double* dv = dgvar + ((size_t)k * ldo + i) * m;
    for (int j = 0; j < d; ++j) {
        dg[j] = s[j] - s[2 * d + 6 + j];
        dv[j] = -D * (2.0 * s[d + j] - rdk[(size_t)j * n0r + i]);
    }
    const double xcz = s[2 * d], xcv = s[2 * d + 1], rz = s[2 * d + 2], rv = s[2 * d + 3], vv = s[2 * d + 4], s2vv = s[2 * d + 5];
    const double xz = fma(scale * nt, rz, xcz), xv = fma(scale * nt, rv, xcv);        // X . z, X . V with the nugget entry
    dg[d] = xz / scale - s[3 * d + 6];
    dv[d] = 1.0 - D * (xv + vv) / scale;
    dg[d + 1] = fma(scale * w1, rz, -xcz * omw) - s[3 * d + 7];
    dv[d + 1] = -D * (2.0 * fma(scale * w1, rv, -xcv * omw) - (D * scale * s2vv - (xv - vv)) * omw);
    const double* vyr = vy + ((size_t)k * n0r + i) * ppad;
    double* dn = dnoise + ((size_t)k * ldo + i) * p;
    for (int a = 0; a < p; ++a) dn[a] = -0.5 * th[d + 3 + a] * vyr[a];
}

// enqueues the pass for the components [k0, k0 + qg) of the workspace; the outputs are those of the q_local components
int do_predict_paramgrad(hipStream_t st, const Ws& w, const void* x, const double* Y, const void* sr, const double* theta, int k0,
                         int qg, int n0, const void* x0, int same, char* scratch, double* ghat, double* gvar, double* dghat,
                         double* dgvar, double* dnoise, int ldo) {
    const int n = w.n, d = w.d, p = w.p, npad = w.npad, tw = d + 3 + p;
    const PgradLay L = pgrad_carve(n, d, p, qg, n0);
    const int m = L.m;
    double* X = (double*)(scratch + L.off_x);          // X, then V
    double* U = (double*)(scratch + L.off_u);          // U, then T_j
    double* E = (double*)(scratch + L.off_e);
    double* XS = (double*)(scratch + L.off_xs);
    double* YV = (double*)(scratch + L.off_yv);
    double* YT = (double*)(scratch + L.off_yt);
    double* VY = (double*)(scratch + L.off_vy);
    double* RD = (double*)(scratch + L.off_rd);
    double* SUM = (double*)(scratch + L.off_sum);
    const double* W = (const double*)(w.base + w.off_W) + (size_t)k0 * w.mat;
    const double* bv = (const double*)(w.base + w.off_b) + (size_t)k0 * npad;
    const double* zv = (const double*)(w.base + w.off_z) + (size_t)k0 * npad;
    const double* th = theta + (size_t)k0 * tw;
    const double* xd = (const double*)x;
    const double* srd = (const double*)sr;
    const double* x0d = (const double*)x0;
    double* gh = ghat + (size_t)k0 * ldo;
    double* gv = gvar + (size_t)k0 * ldo;

    hipLaunchKernelGGL(hess_prep_kernel, dim3((npad + 255) / 256, qg), dim3(256), 0, st, xd, srd, n, npad, d, th, tw, bv, zv, XS, YV);
    CHECK_LAUNCH("hess_prep_kernel");
    // X, U = X W^T, ghat / gvar, V = U W: the launches of lcgp_predict_grad on the group's components
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<double, decltype(kern)::value>), dim3(w.nb, L.n0p / TS, qg), dim3(256), 0, st, X, npad, n0, n, d,
                           x0d, xd, dummy, th, same, srd, L.n0p, npad, tw, L.slab, (const int*)nullptr);
    });
    CHECK_LAUNCH("cross_kernel");
    int rc = launch_pred<double, OP_PRED_U>(st, X, W, U, L.slab, w.mat, npad, L.n0p, w.nb, qg);
    if (rc) return rc;
    hipLaunchKernelGGL((pred_reduce_kernel<double>), dim3(n0, qg), dim3(64), 0, st, (const double*)X, (const double*)U, L.slab, L.slab,
                       npad, n, zv, npad, th, tw, d, ldo, gh, gv);
    CHECK_LAUNCH("pred_reduce_kernel");
    rc = launch_pred<double, OP_PRED_V>(st, U, W, X, L.slab, w.mat, npad, L.n0p, w.nb, qg);
    if (rc) return rc;
    const double* V = X;
    // per dimension: d_jA, y_j = d_jA z, T_j = V d_jA (rows beyond n0p of a slab are never written: their products are never read)
    const dim3 full((npad + 255) / 256, npad, qg);
    GemmArgs g;
    g.A = V; g.B = E; g.C = U; g.ldA = g.ldB = g.ldC = npad;
    g.sA = L.slab; g.sB = L.mat; g.sC = L.slab;
    g.nb = L.nb / 2; g.p0 = L.n0r / (2 * TS); g.p1 = L.nb / 2; g.p2 = g.p3 = 0;
    for (int j = 0; j < d; ++j) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((hess_da_kernel<decltype(kern)::value>), full, dim3(256), 0, st, E, L.mat, n, npad, d, j,
                               (const double*)XS, srd, th, tw);
        });
        CHECK_LAUNCH("hess_da_kernel");
        hipLaunchKernelGGL(hess_matvec_kernel, dim3(npad / 4, 1, qg), dim3(256), 0, st, (const double*)E, L.mat, n, npad, zv, (size_t)npad,
                           YV + (size_t)j * npad, (size_t)m * npad);
        CHECK_LAUNCH("hess_matvec_kernel");
        rc = launch_gemm<double, OP_HESS_G, 128>(st, g, g.p0 * g.nb, qg);
        if (rc) return rc;
        hipLaunchKernelGGL(pgrad_rowdot_kernel, dim3(n0, qg), dim3(64), 0, st, (const double*)U, V, L.slab, npad, n,
                           RD + (size_t)j * L.n0r, (size_t)d * L.n0r);
        CHECK_LAUNCH("pgrad_rowdot_kernel");
    }
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((pgrad_row_kernel<decltype(kern)::value>), dim3(n0, qg, (d + PP_DB - 1) / PP_DB), dim3(256), 0, st, x0d, n0,
                           same, (const double*)XS, srd, n, npad, d, th, tw, zv, V, L.slab, (const double*)YV, SUM, L.n0r, L.nsum);
    });
    CHECK_LAUNCH("pgrad_row_kernel");
    // V Y^T (Y^T zero padded to whole tiles)
    hipLaunchKernelGGL(pgrad_pack_yt_kernel, dim3((L.ppad + 255) / 256, npad), dim3(256), 0, st, Y, p, n, L.ppad, YT);
    CHECK_LAUNCH("pgrad_pack_yt_kernel");
    GemmArgs gy;
    gy.A = V; gy.B = YT; gy.C = VY; gy.ldA = npad; gy.ldB = gy.ldC = L.ppad;
    gy.sA = L.slab; gy.sB = 0; gy.sC = (size_t)L.n0r * L.ppad;
    gy.nb = L.ppad / (2 * TS); gy.p0 = L.n0r / (2 * TS); gy.p1 = L.nb / 2; gy.p2 = gy.p3 = 0;
    rc = launch_gemm<double, OP_HESS_G, 128>(st, gy, gy.p0 * gy.nb, qg);
    if (rc) return rc;
    const size_t ko = (size_t)k0 * ldo;
    hipLaunchKernelGGL(pgrad_final_kernel, dim3((n0 + 255) / 256, qg), dim3(256), 0, st, (const double*)SUM, L.n0r, L.nsum,
                       (const double*)RD, (const double*)VY, L.ppad, n0, d, p, th, tw, ldo, dghat + ko * m, dgvar + ko * m,
                       dnoise + ko * p);
    CHECK_LAUNCH("pgrad_final_kernel");
    return 0;
}

int check_sel(int n_ref, int n_cand, int size) {
    int rc = check_vr(n_ref, n_cand);
    if (rc) return rc;
    if (size < 1 || size > n_cand) return bad("size must be in [1, n_cand]");
    return 0;
}

// host-side checks of the folds (CSR over the n training inputs); returns the largest fold size in *mmax
int check_folds(int n, int q_local, int F, const int* folds, int* mmax) {
    if (F < 1) return bad("F must be >= 1");
    if ((long long)F * q_local > 65535) return bad("F * q_local must be <= 65535");
    if (!folds) return bad("NULL folds_host");
    const int* ptr = folds;
    const int* idx = folds + F + 1;
    if (ptr[0] != 0 || ptr[F] != n) return bad("fold_ptr must start at 0 and end at n");
    std::vector<char> seen((size_t)n, 0);
    int mx = 0;
    for (int f = 0; f < F; ++f) {
        const int m = ptr[f + 1] - ptr[f];
        if (m < 1) return bad("empty fold");
        mx = max(mx, m);
        for (int e = ptr[f]; e < ptr[f + 1]; ++e) {
            const int v = idx[e];
            if (v < 0 || v >= n) return bad("fold index out of range");
            if (seen[v]) return bad("fold index repeated");
            seen[v] = 1;
            if (e > ptr[f] && v < idx[e - 1]) return bad("fold indices must be sorted ascending within a fold");
        }
    }
    *mmax = mx;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// calibration rows (lcgp_calib_rows): per row i the Gaussian log density of one observation vector given the row's latent
// prediction, folded to q-space (include/lcgp_hip.h), with its sensitivities s = d ll / d ghat, v = d ll / d gvar and the
// contraction with the latent Jacobians.  float64; one launch; no atomics; every row is computed from its own inputs in a
// fixed order, so a row's result does not depend on which call or which position it is in.
// M is symmetric (the host symmetrises it): both kernels read M[j * q + k] for M_kj.
// The formulas are evaluated as the header states them (a by back substitution, s = w - M a): the kernels differ from a plain
// float64 evaluation in summation order and fused multiply-adds only.
// ---------------------------------------------------------------------------------------------------

// q <= 8: one thread per row, Q a template parameter and every loop over components unrolled (K, L, the vectors: registers;
// no runtime-indexed array).  M and b are staged once per workgroup in LDS and read as broadcasts.
template <int Q, bool GRAD>
__global__ __launch_bounds__(64) void calib_rows_small_kernel(int d, int n0, const double* __restrict__ ghat,
                                                               const double* __restrict__ gvar, const double* __restrict__ dghat,
                                                               const double* __restrict__ dgvar, size_t ld,
                                                               const double* __restrict__ M, const double* __restrict__ b, double c0,
                                                               double lognorm, const double* __restrict__ inv_range,
                                                               double* __restrict__ ll, double* __restrict__ dll,
                                                               double* __restrict__ sens) {
    __shared__ double sM[Q * Q];
    __shared__ double sb[Q];
    for (int t = threadIdx.x; t < Q * Q; t += 64) sM[t] = M[t];
    if (threadIdx.x < Q) sb[threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n0) return;
    double g[Q], h[Q], w[Q], u[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        g[k] = ghat[(size_t)k * ld + i];
        h[k] = sqrt(fmax(gvar[(size_t)k * ld + i], 0.0));
    }
    double bg = 0.0, gmg = 0.0;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        double mg = 0.0;
#pragma unroll
        for (int j = 0; j < Q; ++j) mg += sM[j * Q + k] * g[j];
        w[k] = sb[k] - mg;
        bg += sb[k] * g[k];
        gmg += g[k] * mg;
    }
    // K = I + diag(h) M diag(h) = L L^T, row by row (only the lower triangle of L is ever touched)
    double L[Q][Q];
    double sumlog = 0.0, uu = 0.0;
#pragma unroll
    for (int r = 0; r < Q; ++r) {
#pragma unroll
        for (int j = 0; j <= r; ++j) {
            double acc = h[r] * sM[j * Q + r] * h[j] + (j == r ? 1.0 : 0.0);
#pragma unroll
            for (int m = 0; m < j; ++m) acc -= L[r][m] * L[j][m];
            L[r][j] = j == r ? sqrt(acc) : acc / L[j][j];
        }
        sumlog += log(L[r][r]);
        double acc = h[r] * w[r];
#pragma unroll
        for (int m = 0; m < r; ++m) acc -= L[r][m] * u[m];
        u[r] = acc / L[r][r];
        uu += u[r] * u[r];
    }
    ll[i] = -0.5 * (c0 - 2.0 * bg + gmg - uu + 2.0 * sumlog + lognorm);
    if (!GRAD && !sens) return;
    // a = h o L^-T u (u is overwritten), then per component s_k = w_k - (M a)_k and column k of R = L^-1 diag(h) M for its
    // squared norm (T_kk = M_kk - |R_k|^2)
#pragma unroll
    for (int j = Q - 1; j >= 0; --j) {
        double acc = u[j];
#pragma unroll
        for (int m = j + 1; m < Q; ++m) acc -= L[m][j] * u[m];
        u[j] = acc / L[j][j];
    }
#pragma unroll
    for (int j = 0; j < Q; ++j) u[j] *= h[j];
    double s[Q], v[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        double y[Q];
        double tk = 0.0, ma = 0.0;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            double acc = h[j] * sM[j * Q + k];
#pragma unroll
            for (int m = 0; m < j; ++m) acc -= L[j][m] * y[m];
            y[j] = acc / L[j][j];
            tk += y[j] * y[j];
            ma += sM[j * Q + k] * u[j];
        }
        s[k] = w[k] - ma;
        v[k] = 0.5 * s[k] * s[k] - 0.5 * (sM[k * Q + k] - tk);
    }
    if (sens) {
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            sens[(size_t)k * n0 + i] = s[k];
            sens[(size_t)(Q + k) * n0 + i] = v[k];
        }
    }
    if (GRAD) {
        for (int l = 0; l < d; ++l) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                const size_t at = ((size_t)k * ld + i) * d + l;
                acc += s[k] * dghat[at] + v[k] * dgvar[at];
            }
            dll[(size_t)i * d + l] = inv_range ? inv_range[l] * acc : acc;
        }
    }
}

// v of lane `lane` (the same lane for the whole wave) in every lane
__device__ __forceinline__ double calib_lane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// acc - sum_{m < n} a[m * q] b[m * q] in four partial sums over m mod 4: chains of n / 4 roundings, not n.  The second launch
// of lcgp_calib_hess_rows solves for R and forms B with it: at q = 64 single chains leave B's tolerance, 4 eps (|M| + |R|^T |R|),
// by a tenth on some rows.  Symmetric in a and b bit for bit.
__device__ __forceinline__ double calib_sub_dot4(double acc, const double* a, const double* b, int q, int n) {
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int m = 0;
    for (; m + 3 < n; m += 4) {
        acc -= a[m * q] * b[m * q];
        a1 -= a[(m + 1) * q] * b[(m + 1) * q];
        a2 -= a[(m + 2) * q] * b[(m + 2) * q];
        a3 -= a[(m + 3) * q] * b[(m + 3) * q];
    }
    for (; m < n; ++m) acc -= a[m * q] * b[m * q];
    return (acc + a1) + (a2 + a3);
}

// 8 < q <= 64: one wavefront (= one workgroup) per row, lane k owns component k: row k of the left-looking Cholesky, then
// column k of R.  Dynamic LDS, 2 q^2 doubles: LT[m * q + k] = L[k][m] (the factor stored transposed: lanes read consecutive
// addresses, the pivot row is a broadcast, so no padding is needed) and R[j * q + k] (diag(h) M, solved in place, each lane
// its own column).  The forward substitution for u rides on the factorisation's steps.
// HESS (lcgp_calib_hess_rows' second launch): the same steps to s, v and R, nothing written to ll / dll / sens; then B = M - R^T R
// takes L's place in LDS (B[j * q + k] = B_kj, lane k its own column; the products R_mk R_mj commute and M is symmetric, so B
// is bitwise symmetric) and per column c <= l of the packed triangle
//     x1 = B P[:, c],  x2 = B (s o V[:, c]),  x3 = (B o B) V[:, c]          (lane k owns entry k; P = dghat, V = dgvar of the row)
//     alpha = -(x1 + x2),  beta = 1/2 x3 - s o (x1 + x2)
//     d2ll[l, c] = inv_range_l inv_range_c sum_k (s_k d2ghat[k, l, c] + v_k d2gvar[k, l, c] + P_kl alpha_k + V_kl beta_k)
// with the lanes striding over l >= c: the four matrix terms of the header folded into two q-vectors per column by B's
// symmetry.  O(q^3) for B, O(q^2 d + q d^2) for the contraction, nothing of size d x d x q^2.
template <bool HESS>
__device__ __forceinline__ void calib_wave_row(int q, int d, int n0, const double* __restrict__ ghat,
                                               const double* __restrict__ gvar, const double* __restrict__ dghat,
                                               const double* __restrict__ dgvar, size_t ld,
                                               const double* __restrict__ M, const double* __restrict__ b, double c0,
                                               double lognorm, const double* __restrict__ inv_range,
                                               double* __restrict__ ll, double* __restrict__ dll,
                                               double* __restrict__ sens, const double* __restrict__ d2ghat,
                                               const double* __restrict__ d2gvar, double* __restrict__ d2ll,
                                               double* __restrict__ Bout) {
    extern __shared__ __attribute__((aligned(16))) char calib_lds[];
    double* LT = (double*)calib_lds;
    double* R = LT + q * q;
    const int k = threadIdx.x;
    const int i = blockIdx.x;
    const bool on = k < q;
    const double g = on ? ghat[(size_t)k * ld + i] : 0.0;
    const double h = on ? sqrt(fmax(gvar[(size_t)k * ld + i], 0.0)) : 0.0;
    const double bk = on ? b[k] : 0.0;
    double mg = 0.0, mkk = 0.0;
    for (int j = 0; j < q; ++j) {
        const double gj = calib_lane(g, j), hj = calib_lane(h, j);
        if (on) {
            const double m = M[j * q + k];
            mg += m * gj;
            R[j * q + k] = hj * m;
            if (j == k) mkk = m;
        }
    }
    const double w = bk - mg;
    const double bg = wave_sum(bk * g), gmg = wave_sum(g * mg);
    double rhs = h * w, u = 0.0, sumlog = 0.0, uu = 0.0;
    for (int j = 0; j < q; ++j) {
        double acc = 0.0;
        if (on && k >= j) {
            acc = h * R[j * q + k] + (j == k ? 1.0 : 0.0);
            for (int m = 0; m < j; ++m) acc -= LT[m * q + k] * LT[m * q + j];
        }
        const double piv = sqrt(calib_lane(acc, j));
        const double lkj = k == j ? piv : acc / piv;
        if (on && k >= j) LT[j * q + k] = lkj;
        sumlog += log(piv);
        const double uj = calib_lane(rhs, j) / piv;
        if (k == j) u = uj;
        if (k > j) rhs -= lkj * uj;
        uu += uj * uj;
        __syncthreads();        // (one wave per workgroup) row j of LT is read by every lane from the next step on
    }
    if (!HESS) {
        if (k == 0) ll[i] = -0.5 * (c0 - 2.0 * bg + gmg - uu + 2.0 * sumlog + lognorm);
        if (!dll && !sens) return;
    }
    // x = L^-T u, one wave sum per step: lane m > j holds its final x_m and reads L[m][j] = LT[j * q + m] (consecutive addresses)
    double xk = 0.0;
    for (int j = q - 1; j >= 0; --j) {
        const double rest = wave_sum(on && k > j ? LT[j * q + k] * xk : 0.0);
        const double xj = (calib_lane(u, j) - rest) / LT[j * q + j];
        if (k == j) xk = xj;
    }
    const double a = h * xk;
    double tk = 0.0, ma = 0.0;
    for (int j = 0; j < q; ++j) {
        const double aj = calib_lane(a, j);
        if (on) {
            ma += M[j * q + k] * aj;
            double acc = R[j * q + k];
            if (HESS) {
                acc = calib_sub_dot4(acc, LT + j, R + k, q, j);
            } else {
                for (int m = 0; m < j; ++m) acc -= LT[m * q + j] * R[m * q + k];
            }
            const double y = acc / LT[j * q + j];
            R[j * q + k] = y;
            tk += y * y;
        }
    }
    const double s = w - ma;
    const double v = 0.5 * s * s - 0.5 * (mkk - tk);
    if (!HESS) {
        if (sens && on) {
            sens[(size_t)k * n0 + i] = s;
            sens[(size_t)(q + k) * n0 + i] = v;
        }
        if (dll) {
            for (int l0 = 0; l0 < d; l0 += 64) {
                const int l = l0 + k;
                double acc = 0.0;
                for (int c = 0; c < q; ++c) {
                    const double sc = calib_lane(s, c), vc = calib_lane(v, c);
                    if (l < d) {
                        const size_t at = ((size_t)c * ld + i) * d + l;
                        acc += sc * dghat[at] + vc * dgvar[at];
                    }
                }
                if (l < d) dll[(size_t)i * d + l] = inv_range ? inv_range[l] * acc : acc;
            }
        }
        return;
    }
    __syncthreads();            // R is complete and L is dead: B takes L's place
    double* B = LT;
    if (on) {
        for (int j = 0; j < q; ++j) {
            const double acc = calib_sub_dot4(M[j * q + k], R + k, R + j, q, q);
            B[j * q + k] = acc;
            if (Bout) Bout[((size_t)i * q + j) * q + k] = acc;
        }
    }
    __syncthreads();
    if (!d2ll) return;
    const int tri = d * (d + 1) / 2;
    for (int c = 0; c < d; ++c) {
        const size_t at = ((size_t)k * ld + i) * d + c;
        const double pc = on ? dghat[at] : 0.0, vc = on ? dgvar[at] : 0.0;
        const double sv = s * vc;
        double x1 = 0.0, x2 = 0.0, x3 = 0.0;
        for (int j = 0; j < q; ++j) {
            const double pj = calib_lane(pc, j), svj = calib_lane(sv, j), vj = calib_lane(vc, j);
            if (on) {
                const double bkj = B[j * q + k];
                x1 += bkj * pj;
                x2 += bkj * svj;
                x3 += bkj * bkj * vj;
            }
        }
        const double alpha = -(x1 + x2);
        const double beta = 0.5 * x3 - s * (x1 + x2);
        const double irc = inv_range ? inv_range[c] : 1.0;
        for (int l0 = c; l0 < d; l0 += 64) {
            const int l = l0 + k;
            const bool in = l < d;
            const size_t pk = (size_t)l * (l + 1) / 2 + c;
            double acc = 0.0;
            for (int j = 0; j < q; ++j) {
                const double sj = calib_lane(s, j), vj = calib_lane(v, j);
                if (in) {
                    const size_t ah = ((size_t)j * ld + i) * tri + pk;
                    acc += sj * d2ghat[ah] + vj * d2gvar[ah];
                }
            }
            for (int j = 0; j < q; ++j) {
                const double aj = calib_lane(alpha, j), bj = calib_lane(beta, j);
                if (in) {
                    const size_t aj1 = ((size_t)j * ld + i) * d + l;
                    acc += dghat[aj1] * aj + dgvar[aj1] * bj;
                }
            }
            if (in) d2ll[(size_t)i * tri + pk] = (inv_range ? inv_range[l] * irc : 1.0) * acc;
        }
    }
}

__global__ __launch_bounds__(64) void calib_rows_wave_kernel(int q, int d, int n0, const double* __restrict__ ghat,
                                                              const double* __restrict__ gvar, const double* __restrict__ dghat,
                                                              const double* __restrict__ dgvar, size_t ld,
                                                              const double* __restrict__ M, const double* __restrict__ b, double c0,
                                                              double lognorm, const double* __restrict__ inv_range,
                                                              double* __restrict__ ll, double* __restrict__ dll,
                                                              double* __restrict__ sens) {
    calib_wave_row<false>(q, d, n0, ghat, gvar, dghat, dgvar, ld, M, b, c0, lognorm, inv_range, ll, dll, sens, nullptr, nullptr,
                          nullptr, nullptr);
}

// lcgp_calib_hess_rows' second launch: one wavefront per row for every q in [1, 64]
__global__ __launch_bounds__(64) void calib_hess_wave_kernel(int q, int d, int n0, const double* __restrict__ ghat,
                                                              const double* __restrict__ gvar, const double* __restrict__ dghat,
                                                              const double* __restrict__ dgvar, size_t ld,
                                                              const double* __restrict__ M, const double* __restrict__ b,
                                                              const double* __restrict__ inv_range,
                                                              const double* __restrict__ d2ghat, const double* __restrict__ d2gvar,
                                                              double* __restrict__ d2ll, double* __restrict__ Bout) {
    calib_wave_row<true>(q, d, n0, ghat, gvar, dghat, dgvar, ld, M, b, 0.0, 0.0, inv_range, nullptr, nullptr, nullptr, d2ghat,
                         d2gvar, d2ll, Bout);
}

template <int Q>
int launch_calib_small(hipStream_t st, int d, int n0, const double* ghat, const double* gvar, const double* dghat,
                       const double* dgvar, size_t ld, const double* M, const double* b, double c0, double lognorm,
                       const double* inv_range, double* ll, double* dll, double* sens) {
    const dim3 grid((n0 + 63) / 64), block(64);
    if (dll)
        hipLaunchKernelGGL((calib_rows_small_kernel<Q, true>), grid, block, 0, st, d, n0, ghat, gvar, dghat, dgvar, ld, M, b, c0,
                           lognorm, inv_range, ll, dll, sens);
    else
        hipLaunchKernelGGL((calib_rows_small_kernel<Q, false>), grid, block, 0, st, d, n0, ghat, gvar, dghat, dgvar, ld, M, b, c0,
                           lognorm, inv_range, ll, dll, sens);
    CHECK_LAUNCH("calib_rows_small");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Sobol indices of the posterior mean surface in closed form (lcgp_sobol_pairs).  For two components k, k' with
// weight vectors w, w' and one input dimension l, besides the box average a_l[i] of the 1-D factor (marg_I1) the PAIR average
//   J_l[i, i'] = (1 / w_l) int_box kappa(|t - x_il| / ell_kl) kappa(|t - x_i'l| / ell_k'l) dt
// of two factors with different centres and length scales.  SE: the product of two Gaussians is a Gaussian (erf / erfc as in
// marg_I1).  Matern: kappa(s) = P(s) e^-s; the centres are ordered (u <= v), the box split at those inside it into (at most)
// three segments, and on a segment neither t - u nor t - v changes sign, so the integrand is a polynomial times e^(c t).  Each
// segment is anchored at the end where the exponent is largest (t = t0 +- tau) and integrated as
//   e^(-s0a - s0b) sum_n q_n m_n(|c|, L),     m_n(g, L) = int_0^L tau^n e^(-g tau) dtau,
// s0a, s0b the scaled distances at the anchor, q the product of the two polynomials P(s0 +- tau / ell) in powers of tau.  On
// the middle segment g = |1 / a - 1 / b|, which is 0 for equal length scales (every pair k = k'): m_n never divides by g where
// g L is small.  Below g L = 4 the TOP moment comes from the all-positive series
//   m_N = e^(-g L) L^(N + 1) / (N + 1) (1 + x / (N + 2) (1 + x / (N + 3) (1 + ...))),   x = g L,   30 terms (the first one left
// out is below 1e-18 of the sum), the lower ones from the backward recurrence m_(n-1) = (g m_n + L^n e^(-g L)) / n (all
// positive as well, exact at g = 0); from 4 on m_0 = -expm1(-g L) / g and the forward recurrence m_n = (n m_(n-1) - L^n
// e^(-g L)) / g, whose error amplification n / (g L) stays below 1 there (n <= 4).
// ---------------------------------------------------------------------------------------------------
constexpr double SOBOL_SERIES_BELOW = 4.0;
constexpr int SOBOL_SERIES_TERMS = 30;
constexpr int SOBOL_BATCH = 64;               // pairs per launch (their component indices travel as kernel arguments)

struct SobolPairs { int k[SOBOL_BATCH], kp[SOBOL_BATCH]; };

// what one input dimension contributes to every J of a pair: the box and per kernel the constants of the two length scales
//   Matern: c0 = 1 / a, c1 = 1 / b.   SE (s2 = a^2 + b^2): c0 = -1 / (2 s2), c1 = sigma = a b / sqrt(s2), c2 = 1 / sigma,
//   c3 = b^2 / s2, c4 = a^2 / s2 (the centre of the product is c3 u + c4 v)
struct SobolDim { double lo, hi, rw, c0, c1, c2, c3, c4; };

template <int KERN>
__device__ __forceinline__ SobolDim sobol_dim(double a, double b, double lo, double hi) {
    static_assert(kern_known<KERN>::value, "unknown covariance kernel id");
    SobolDim c;
    c.lo = lo; c.hi = hi; c.rw = 1.0 / (hi - lo);
    if constexpr (KERN == 1) {
        const double s2 = a * a + b * b;
        c.c0 = -0.5 / s2;
        c.c1 = a * b / sqrt(s2);
        c.c2 = 1.0 / c.c1;
        c.c3 = b * b / s2;
        c.c4 = a * a / s2;
    } else {
        c.c0 = 1.0 / a; c.c1 = 1.0 / b; c.c2 = c.c3 = c.c4 = 0.0;
    }
    return c;
}

// m[n] = int_0^L tau^n e^(-g tau) dtau, n = 0 .. NT (g >= 0, L >= 0)
template <int NT>
__device__ __forceinline__ void sobol_moments(double g, double L, double (&m)[NT + 1]) {
    const double x = g * L;
    const double eL = exp(-x);
    double Ln[NT + 2];                                     // L^n
    Ln[0] = 1.0;
#pragma unroll
    for (int n = 1; n <= NT + 1; ++n) Ln[n] = Ln[n - 1] * L;
    if (x < SOBOL_SERIES_BELOW) {
        double s = 1.0;
#pragma unroll
        for (int j = SOBOL_SERIES_TERMS; j >= 1; --j) s = fma(s * x, 1.0 / (NT + 1 + j), 1.0);
        m[NT] = eL * Ln[NT + 1] * s * (1.0 / (NT + 1));
#pragma unroll
        for (int n = NT; n >= 1; --n) m[n - 1] = fma(g, m[n], Ln[n] * eL) * (1.0 / n);
    } else {
        const double rg = fast_rcp(g);
        m[0] = -expm1(-x) * rg;
#pragma unroll
        for (int n = 1; n <= NT; ++n) m[n] = fma((double)n, m[n - 1], -Ln[n] * eL) * rg;
    }
}

// one segment of length L: e^(-s0a - s0b) sum_n q_n m_n(al + be, L), with P(s0a + al tau) P(s0b + be tau) = sum_n q_n tau^n
template <int KERN>
__device__ __forceinline__ double sobol_segment(double L, double s0a, double s0b, double al, double be) {
    constexpr int NT = KERN == 0 ? 2 : 4;
    double m[NT + 1];
    sobol_moments<NT>(al + be, L, m);
    double sum;
    if constexpr (KERN == 0) {
        const double a0 = 1.0 + s0a, b0 = 1.0 + s0b;
        sum = a0 * b0 * m[0] + fma(a0, be, al * b0) * m[1] + al * be * m[2];
    } else {
        const double a0 = 1.0 + fma(s0a * (1.0 / 3.0), s0a, s0a), a1 = al * fma(s0a, 2.0 / 3.0, 1.0), a2 = al * al * (1.0 / 3.0);
        const double b0 = 1.0 + fma(s0b * (1.0 / 3.0), s0b, s0b), b1 = be * fma(s0b, 2.0 / 3.0, 1.0), b2 = be * be * (1.0 / 3.0);
        sum = a0 * b0 * m[0] + fma(a0, b1, a1 * b0) * m[1] + (fma(a0, b2, a2 * b0) + a1 * b1) * m[2] + fma(a1, b2, a2 * b1) * m[3] +
              a2 * b2 * m[4];
    }
    return exp(-(s0a + s0b)) * sum;
}

// J = (1 / w) int_lo^hi kappa(|t - u| / a) kappa(|t - v| / b) dt
template <int KERN>
__device__ __forceinline__ double sobol_J(double u, double v, const SobolDim& c) {
    if constexpr (KERN == 1) {
        const double df = u - v;
        const double pref = exp(c.c0 * df * df);
        const double mu = fma(c.c3, u, c.c4 * v);
        const double z1 = (mu - c.lo) * c.c2, z2 = (c.hi - mu) * c.c2;
        const double b1 = fabs(z1), b2 = fabs(z2);
        double r;
        if (z1 >= 0.0 && z2 >= 0.0) {
            r = marg_F<1>(b1) + marg_F<1>(b2);
        } else {
            const double bn = fmin(b1, b2), bf = fmax(b1, b2);
            r = bn > 1.0 ? marg_Fc<1>(bn) - marg_Fc<1>(bf) : marg_F<1>(bf) - marg_F<1>(bn);
        }
        return pref * c.c1 * r * c.rw;
    } else {
        double ra = c.c0, rb = c.c1;
        if (u > v) {
            const double t = u; u = v; v = t;
            ra = c.c1; rb = c.c0;
        }
        const double cu = fmin(fmax(u, c.lo), c.hi), cv = fmin(fmax(v, c.lo), c.hi);
        // (a centre outside the box leaves segments of length 0: their moments are 0, and the distances below are taken as
        // absolute values so that the factor in front stays finite)
        // left of both centres: anchored at its right end, both distances grow with tau
        double tot = sobol_segment<KERN>(cu - c.lo, fabs(u - cu) * ra, fabs(v - cu) * rb, ra, rb);
        // between the centres: anchored at the end with the larger exponent, the centre with the shorter length scale
        if (rb <= ra) tot += sobol_segment<KERN>(cv - cu, fabs(cu - u) * ra, fabs(v - cu) * rb, ra, -rb);
        else tot += sobol_segment<KERN>(cv - cu, fabs(cv - u) * ra, fabs(v - cv) * rb, -ra, rb);
        // right of both: anchored at its left end
        tot += sobol_segment<KERN>(c.hi - cv, fabs(cv - u) * ra, fabs(cv - v) * rb, ra, rb);
        return tot * c.rw;
    }
}

__device__ __forceinline__ double sobol_wave_sum(double v) {          // lane 0 holds the sum; a fixed order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the matrix a matrix-weighted pair launch reads its weights from: component k's at base + k * mat, rows of npad doubles, the
// lower triangle valid (the A^-1 slot of a float64 workspace); all zero in the launches of lcgp_sobol_pairs, which never read it
struct SobolQ {
    const double* base; size_t mat; int npad;
    // SOBOL_VIEW only (lcgp_condition_sobol_matrix_pairs): the plane is (nt + m) x (nt + m); the second source E
    // (ONE component's, rows of epad doubles, lower tiles valid) covers all of it, `base` its leading nt x nt block, times *dk
    const double* e = nullptr; int epad = 0, nt = 0; const double* dk = nullptr;
};

// where the weight of an element comes from: the product of two vectors (lcgp_sobol_pairs), times an entry of A^-1
// (lcgp_sobol_matrix_pairs), times E[i, i'] + D A^-1[i, i'] (i, i' < nt) on a conditioned view
enum SobolWeight { SOBOL_VEC = 0, SOBOL_MAT = 1, SOBOL_VIEW = 2 };

// tile (r, c), c <= r, of component k's matrix into qt[i * (TS + 1) + j], for the 256 threads of a workgroup: thread e reads
// row e / 64, column e % 64, so a wavefront reads 64 consecutive doubles of one row.  In a diagonal tile only j <= i is read
// and written to both (i, j) and (j, i): an element above the diagonal takes the mirrored entry.  Rows and columns beyond n
// (never used by the element loop) are zero.  The caller's barrier follows.
// SOBOL_VIEW: the element is E[gi, gj] (gi, gj < n = nt + m) plus D A^-1[gi, gj] where both indices are below nt; the boundary nt
// may cut a tile, a diagonal one too: the sum is formed before the mirrored write, so the mirror holds for both sources.
template <int MAT>
__device__ __forceinline__ void sobol_stage_q(double* qt, const SobolQ& qm, int k, int n, int r, int c, int tid) {
    const double* src = qm.base + (size_t)k * qm.mat;
    [[maybe_unused]] double dk = 0.0;
    if constexpr (MAT == SOBOL_VIEW) dk = *qm.dk;
    for (int e = tid; e < TS * TS; e += 256) {
        const int i = e >> 6, j = e & 63;
        const int gi = r * TS + i, gj = c * TS + j;
        if (r == c && j > i) continue;
        double v;
        if constexpr (MAT == SOBOL_VIEW) {
            v = (gi < n && gj < n) ? qm.e[(size_t)gi * qm.epad + gj] : 0.0;
            if (gi < qm.nt && gj < qm.nt) v = fma(dk, src[(size_t)gi * qm.npad + gj], v);
        } else {
            v = (gi < n && gj < n) ? src[(size_t)gi * qm.npad + gj] : 0.0;
        }
        qt[i * (TS + 1) + j] = v;
        if (r == c) qt[j * (TS + 1) + i] = v;
    }
}

// launch 1: tab[k, l, i] = the box average of the 1-D factor of component k at training input i (marg_I1), and the box mean
// means[k] = sum_i w_ki prod_l tab[k, l, i] of the component's surface, reduced in a fixed order.  One workgroup per component.
template <int KERN>
__global__ __launch_bounds__(256) void sobol_table_kernel(const double* __restrict__ x, int n, int d, const double* __restrict__ w,
                                                          const double* __restrict__ ell, const double* __restrict__ box,
                                                          double* __restrict__ tab, double* __restrict__ means) {
    __shared__ double red[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n; i += 256) {
        double pr = 1.0;
        for (int l = 0; l < d; ++l) {
            const double v = marg_I1<KERN>(x[(size_t)i * d + l], box[l], box[d + l], ell[(size_t)k * d + l]);
            tab[((size_t)k * d + l) * n + i] = v;
            pr *= v;
        }
        acc = fma(w[(size_t)k * n + i], pr, acc);
    }
    acc = sobol_wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) means[k] = (red[0] + red[1]) + (red[2] + red[3]);
}

// launch 2: one 64 x 64 tile of the (i, i') plane of one pair per workgroup, 16 elements per thread, one after the other.  Per
// element the d pair averages J_l (a rolled loop: the code of one J is long) go through the thread's own LDS column into
// registers, the d products A_l = a_l[i] a'_l[i'] beside them; prefix and suffix products then give the 2 d + 1 subset products
// M_u without a division (factors underflow to zero), and w_i w'_i' (M_u - M_0) is accumulated per subset: the difference is
// taken per element, never between two large sums.  Rows and columns beyond n are skipped.  A pair k = k' visits the tiles with
// column tile <= row tile and counts the strictly lower ones twice.  The block sums go to part[pair, tile, subset] (wave
// shuffles, then the four waves in order): no atomics.  DD >= d bounds the unrolled loops.
// MAT (lcgp_sobol_matrix_pairs): pairs k = k' of LOCAL components only, and the weight of an element is
// w_i w_i' Q[i, i'] with Q the component's matrix in `qm` (A^-1 in place: qmat elements per component, rows of npad, its lower
// triangle valid).  The tile of Q goes through LDS (sobol_stage_q); one more sum per tile, S0 = sum w_i w_i' Q M_0, follows the
// 2 d + 1 others in part.  Nothing of MAT is instantiated in the instances without it.
template <int KERN, int DD, int MAT>
__global__ __launch_bounds__(256) void sobol_pair_kernel(const double* __restrict__ x, int n, int d, const double* __restrict__ w,
                                                         const double* __restrict__ ell, const double* __restrict__ box,
                                                         const double* __restrict__ tab, SobolPairs pr, int ntile,
                                                         double* __restrict__ part, SobolQ qm) {
    __shared__ double xr[TS][DD + 1], xc[TS][DD + 1], ar[TS][DD + 1], ac[TS][DD + 1];
    __shared__ double wr[TS], wc[TS];
    __shared__ double Js[DD][256];
    __shared__ SobolDim cst[DD];
    __shared__ double red[4][2 * DD + (MAT ? 2 : 1)];
    const int r = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const int k = pr.k[z], kp = pr.kp[z];
    if (k == kp && c > r) return;
    const int tid = threadIdx.x;
    for (int e = tid; e < TS * DD; e += 256) {
        const int i = e / DD, l = e - i * DD;
        const int gi = r * TS + i, gj = c * TS + i;
        const bool vi = gi < n && l < d, vj = gj < n && l < d;
        xr[i][l] = vi ? x[(size_t)gi * d + l] : 0.0;
        xc[i][l] = vj ? x[(size_t)gj * d + l] : 0.0;
        ar[i][l] = vi ? tab[((size_t)k * d + l) * n + gi] : 1.0;
        ac[i][l] = vj ? tab[((size_t)kp * d + l) * n + gj] : 1.0;
    }
    if (tid < TS) {
        const int gi = r * TS + tid, gj = c * TS + tid;
        wr[tid] = gi < n ? w[(size_t)k * n + gi] : 0.0;
        wc[tid] = gj < n ? w[(size_t)kp * n + gj] : 0.0;
    }
    if (tid < DD) {
        if (tid < d) cst[tid] = sobol_dim<KERN>(ell[(size_t)k * d + tid], ell[(size_t)kp * d + tid], box[tid], box[d + tid]);
    }
#pragma unroll
    for (int l = 0; l < DD; ++l) Js[l][tid] = 1.0;         // (dimensions d .. DD - 1 stay neutral)
    const double* qs = nullptr;
    if constexpr (MAT) {
        __shared__ double qtile[TS * (TS + 1)];
        sobol_stage_q<MAT>(qtile, qm, k, n, r, c, tid);
        qs = qtile;
    }
    __syncthreads();
    const double twice = (k == kp && c < r) ? 2.0 : 1.0;
    const int tx = tid & 15, ty = tid >> 4;
    double accF[DD], accC[DD], accA = 0.0;
    [[maybe_unused]] double accS = 0.0;
#pragma unroll
    for (int l = 0; l < DD; ++l) accF[l] = accC[l] = 0.0;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int i = ty * 4 + (e >> 2), j = tx + 16 * (e & 3);
        if (r * TS + i >= n || c * TS + j >= n) continue;
#pragma unroll 1
        for (int l = 0; l < d; ++l) Js[l][tid] = sobol_J<KERN>(xr[i][l], xc[j][l], cst[l]);
        // the weight of the element: ONE place (a matrix entry can take the product's place)
        double wgt = twice * (wr[i] * wc[j]);
        if constexpr (MAT) wgt *= qs[i * (TS + 1) + j];
        double J[DD], A[DD], F[DD], Cl[DD];
        double pa = 1.0, pj = 1.0;
#pragma unroll
        for (int l = 0; l < DD; ++l) {
            J[l] = Js[l][tid];
            A[l] = ar[i][l] * ac[j][l];
            F[l] = pa * J[l];
            Cl[l] = pj * A[l];
            pa *= A[l];
            pj *= J[l];
        }
        const double m0 = pa;
        accA = fma(wgt, pj - m0, accA);
        if constexpr (MAT) accS = fma(wgt, m0, accS);
        double sa = 1.0, sj = 1.0;
#pragma unroll
        for (int l = DD - 1; l >= 0; --l) {
            accF[l] = fma(wgt, F[l] * sa - m0, accF[l]);
            accC[l] = fma(wgt, Cl[l] * sj - m0, accC[l]);
            sa *= A[l];
            sj *= J[l];
        }
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int l = 0; l < DD; ++l) {
        const double f = sobol_wave_sum(accF[l]), g = sobol_wave_sum(accC[l]);
        if (lane == 0 && l < d) { red[wave][l] = f; red[wave][d + l] = g; }
    }
    accA = sobol_wave_sum(accA);
    if (lane == 0) red[wave][2 * d] = accA;
    if constexpr (MAT) {
        accS = sobol_wave_sum(accS);
        if (lane == 0) red[wave][2 * d + 1] = accS;
    }
    __syncthreads();
    constexpr int EX = MAT ? 1 : 0;
    if (tid < 2 * d + 1 + EX)
        part[(((size_t)z * ntile + r) * ntile + c) * (2 * d + 1 + EX) + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// launch 2 for d > 16: the same tiles, elements and sums, one input l at a time, its three products recomputed from the inputs
// (O(d^2) pair averages per element), nothing staged
template <int KERN, int MAT>
__global__ __launch_bounds__(256) void sobol_pair_wide_kernel(const double* __restrict__ x, int n, int d, const double* __restrict__ w,
                                                              const double* __restrict__ ell, const double* __restrict__ box,
                                                              const double* __restrict__ tab, SobolPairs pr, int ntile,
                                                              double* __restrict__ part, SobolQ qm) {
    constexpr int NR = MAT ? 4 : 3;                        // sums per round: F, C, all[, S0]
    __shared__ double red[4][NR];
    const int r = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const int k = pr.k[z], kp = pr.kp[z];
    if (k == kp && c > r) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double twice = (k == kp && c < r) ? 2.0 : 1.0;
    const int tx = tid & 15, ty = tid >> 4;
    double* dst = part + (((size_t)z * ntile + r) * ntile + c) * (2 * d + NR - 2);
    const double* qs = nullptr;
    if constexpr (MAT) {                                   // (the one thing staged: every round reads the same weights)
        __shared__ double qtile[TS * (TS + 1)];
        sobol_stage_q<MAT>(qtile, qm, k, n, r, c, tid);
        qs = qtile;
        __syncthreads();
    }
    for (int l = 0; l < d; ++l) {
        double accF = 0.0, accC = 0.0, accA = 0.0;
        [[maybe_unused]] double accS = 0.0;
        for (int e = 0; e < 16; ++e) {
            const int gi = r * TS + ty * 4 + (e >> 2), gj = c * TS + tx + 16 * (e & 3);
            if (gi >= n || gj >= n) continue;
            double m0 = 1.0, ax = 1.0, jx = 1.0, Al = 1.0, Jl = 1.0;       // prod A, prod over m != l of A and of J, A_l, J_l
            for (int m = 0; m < d; ++m) {
                const SobolDim cm = sobol_dim<KERN>(ell[(size_t)k * d + m], ell[(size_t)kp * d + m], box[m], box[d + m]);
                const double Jm = sobol_J<KERN>(x[(size_t)gi * d + m], x[(size_t)gj * d + m], cm);
                const double Am = tab[((size_t)k * d + m) * n + gi] * tab[((size_t)kp * d + m) * n + gj];
                m0 *= Am;
                if (m == l) { Al = Am; Jl = Jm; }
                else { ax *= Am; jx *= Jm; }
            }
            double wgt = twice * (w[(size_t)k * n + gi] * w[(size_t)kp * n + gj]);
            if constexpr (MAT) wgt *= qs[(ty * 4 + (e >> 2)) * (TS + 1) + tx + 16 * (e & 3)];
            accF = fma(wgt, Jl * ax - m0, accF);
            accC = fma(wgt, Al * jx - m0, accC);
            accA = fma(wgt, Jl * jx - m0, accA);
            if constexpr (MAT) accS = fma(wgt, m0, accS);
        }
        accF = sobol_wave_sum(accF);
        accC = sobol_wave_sum(accC);
        accA = sobol_wave_sum(accA);
        if constexpr (MAT) accS = sobol_wave_sum(accS);
        __syncthreads();                                   // (the previous round's sums have been read)
        if (lane == 0) { red[wave][0] = accF; red[wave][1] = accC; red[wave][2] = accA; }
        if constexpr (MAT) {
            if (lane == 0) red[wave][3] = accS;
        }
        __syncthreads();
        if (tid < NR && (tid < 2 || l == 0))
            dst[tid == 0 ? l : tid == 1 ? d + l : 2 * d + tid - 2] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

// launch 3: out[pair, s] = the sum over the pair's tiles of part[pair, tile, s] in a fixed order (thread t adds tiles t, t + 256,
// ..., then a tree over the threads), s = 0 .. 2 d; out[pair, 2 d + 1] = the box mean of component k where k = k', else 0.
// grid (2 d + 2, pairs of the launch).  MAT: part holds 2 d + 2 sums per tile and out[pair, 2 d + 1] is the last one's sum, S0.
template <int MAT>
__global__ __launch_bounds__(256) void sobol_reduce_kernel(const double* __restrict__ part, int ntile, int d, SobolPairs pr,
                                                           const double* __restrict__ means, double* __restrict__ out) {
    __shared__ double red[256];
    const int s = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
    const int k = pr.k[z], kp = pr.kp[z];
    double* dst = out + (size_t)z * (2 * d + 2);
    if constexpr (!MAT) {
        if (s == 2 * d + 1) {
            if (tid == 0) dst[s] = k == kp ? means[k] : 0.0;
            return;
        }
    }
    double acc = 0.0;
    for (int t = tid; t < ntile * ntile; t += 256) {
        const int r = t / ntile, c = t - r * ntile;
        if (k == kp && c > r) continue;
        acc += part[((size_t)z * ntile * ntile + t) * (2 * d + (MAT ? 2 : 1)) + s];
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) dst[s] = red[0];
}

inline size_t sobol_part_doubles(int n, int d, int npairs, int per_tile_extra = 0) {
    const size_t ntile = (n + TS - 1) / TS;
    return (size_t)(npairs < SOBOL_BATCH ? npairs : SOBOL_BATCH) * ntile * ntile * (2 * d + 1 + per_tile_extra);
}

// launches 2 and 3 for the nb <= SOBOL_BATCH pairs in pr: the pair tiles into part, their sums into out (nb rows).  The
// reduction of SOBOL_VIEW is SOBOL_MAT's (2 d + 2 sums per tile either way).
template <int MAT>
int sobol_pair_launches(hipStream_t st, int kern, int n, int d, const double* x, const double* w, const double* ell,
                        const double* box, const double* tab, const double* means, const SobolPairs& pr, int nb, double* part,
                        double* out, const SobolQ& qm) {
    const int ntile = (n + TS - 1) / TS;
    const dim3 grid(ntile, ntile, nb);
    for_kern(kern, [&](auto kn) {
        constexpr int K = decltype(kn)::value;
        if (d <= 8)
            hipLaunchKernelGGL((sobol_pair_kernel<K, 8, MAT>), grid, dim3(256), 0, st, x, n, d, w, ell, box, tab, pr, ntile, part, qm);
        else if (d <= 16)
            hipLaunchKernelGGL((sobol_pair_kernel<K, 16, MAT>), grid, dim3(256), 0, st, x, n, d, w, ell, box, tab, pr, ntile, part, qm);
        else
            hipLaunchKernelGGL((sobol_pair_wide_kernel<K, MAT>), grid, dim3(256), 0, st, x, n, d, w, ell, box, tab, pr, ntile, part, qm);
    });
    CHECK_LAUNCH("sobol_pair_kernel");
    constexpr int RED = MAT == SOBOL_VIEW ? (int)SOBOL_MAT : MAT;
    hipLaunchKernelGGL((sobol_reduce_kernel<RED>), dim3(2 * d + 2, nb), dim3(256), 0, st, part, ntile, d, pr, means, out);
    CHECK_LAUNCH("sobol_reduce_kernel");
    return 0;
}

// SOBOL_VEC: lcgp_sobol_pairs (qm unused).  SOBOL_MAT: lcgp_sobol_matrix_pairs, `pairs` holds (k, k) of local components,
// w their row vectors v and out[pair, 2 d + 1] is S0
template <int MAT>
int do_sobol_pairs(hipStream_t st, int kern, int n, int d, int q_all, const double* x, const double* w, const double* ell,
                   const double* box, const int* pairs, int npairs, void* scratch, double* out, SobolQ qm) {
    double* tab = (double*)scratch;
    double* means = tab + (size_t)q_all * d * n;
    double* part = means + q_all;
    for_kern(kern, [&](auto kn) {
        hipLaunchKernelGGL((sobol_table_kernel<decltype(kn)::value>), dim3(q_all), dim3(256), 0, st, x, n, d, w, ell, box, tab, means);
    });
    CHECK_LAUNCH("sobol_table_kernel");
    for (int p0 = 0; p0 < npairs; p0 += SOBOL_BATCH) {
        const int nb = npairs - p0 < SOBOL_BATCH ? npairs - p0 : SOBOL_BATCH;
        SobolPairs pr;
        for (int i = 0; i < SOBOL_BATCH; ++i) {
            pr.k[i] = i < nb ? pairs[2 * (p0 + i)] : 0;
            pr.kp[i] = i < nb ? pairs[2 * (p0 + i) + 1] : 0;
        }
        int rc = sobol_pair_launches<MAT>(st, kern, n, d, x, w, ell, box, tab, means, pr, nb, part, out + (size_t)p0 * (2 * d + 2), qm);
        if (rc) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The same pass for a caller's list of input subsets (lcgp_sobol_subset_pairs and its two matrix-weighted forms):
// second-order indices, indices of groups, Shapley effects.  What an element costs -- its d pair averages J_l -- does not depend
// on the subset, so one launch accumulates a CHUNK of SC subsets over the J_l it has formed; further chunks are further launches
// that form them again.  A subset travels as a bit mask (bit l: input l is in u), the chunk as a kernel argument: uniform over
// the launch, so every select below is on a scalar condition.
// ---------------------------------------------------------------------------------------------------
template <int SC>
struct SobolMasks { unsigned m[SC]; };

// launch 2 of the subset pass: sobol_pair_kernel's staging, tiles and element loop (the rolled J loop through the thread's LDS
// column); per element and mask s < ns the product P_u = prod_l (bit_l ? J_l : A_l), l ascending (sobol_subset.h: a select per
// factor, no division, nothing contracted), and acc[s] += wgt (P_u - M_0) with M_0 the same product of the A_l alone -- the empty
// mask adds exactly 0.  The weight enters in one place; a pair k = k' visits the lower tiles and counts the strictly lower ones
// twice; rows and columns beyond n are skipped.  The SC accumulators are registers (the mask loop is unrolled: no runtime index
// into them); slot s sees the same instructions whatever the other slots hold, so a mask's sum does not depend on its place in
// the list.  The block sums go to part[pair, tile, s], s < SC (wave shuffles, then the four waves in order): no atomics.
template <int KERN, int DD, int MAT>
__global__ __launch_bounds__(256) void sobol_subset_kernel(const double* __restrict__ x, int n, int d, const double* __restrict__ w,
                                                           const double* __restrict__ ell, const double* __restrict__ box,
                                                           const double* __restrict__ tab, SobolPairs pr, int ntile,
                                                           double* __restrict__ part, SobolQ qm,
                                                           SobolMasks<sobol_subset_chunk(DD)> mk, int ns) {
    constexpr int SC = sobol_subset_chunk(DD);
    __shared__ double xr[TS][DD + 1], xc[TS][DD + 1], ar[TS][DD + 1], ac[TS][DD + 1];
    __shared__ double wr[TS], wc[TS];
    __shared__ double Js[DD][256];
    __shared__ SobolDim cst[DD];
    __shared__ double red[4][SC];
    const int r = blockIdx.x, c = blockIdx.y, z = blockIdx.z;
    const int k = pr.k[z], kp = pr.kp[z];
    if (k == kp && c > r) return;
    const int tid = threadIdx.x;
    for (int e = tid; e < TS * DD; e += 256) {
        const int i = e / DD, l = e - i * DD;
        const int gi = r * TS + i, gj = c * TS + i;
        const bool vi = gi < n && l < d, vj = gj < n && l < d;
        xr[i][l] = vi ? x[(size_t)gi * d + l] : 0.0;
        xc[i][l] = vj ? x[(size_t)gj * d + l] : 0.0;
        ar[i][l] = vi ? tab[((size_t)k * d + l) * n + gi] : 1.0;
        ac[i][l] = vj ? tab[((size_t)kp * d + l) * n + gj] : 1.0;
    }
    if (tid < TS) {
        const int gi = r * TS + tid, gj = c * TS + tid;
        wr[tid] = gi < n ? w[(size_t)k * n + gi] : 0.0;
        wc[tid] = gj < n ? w[(size_t)kp * n + gj] : 0.0;
    }
    if (tid < DD) {
        if (tid < d) cst[tid] = sobol_dim<KERN>(ell[(size_t)k * d + tid], ell[(size_t)kp * d + tid], box[tid], box[d + tid]);
    }
#pragma unroll
    for (int l = 0; l < DD; ++l) Js[l][tid] = 1.0;         // (dimensions d .. DD - 1 stay neutral)
    const double* qs = nullptr;
    if constexpr (MAT) {
        __shared__ double qtile[TS * (TS + 1)];
        sobol_stage_q<MAT>(qtile, qm, k, n, r, c, tid);
        qs = qtile;
    }
    __syncthreads();
    const double twice = (k == kp && c < r) ? 2.0 : 1.0;
    const int tx = tid & 15, ty = tid >> 4;
    double acc[SC];
#pragma unroll
    for (int s = 0; s < SC; ++s) acc[s] = 0.0;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int i = ty * 4 + (e >> 2), j = tx + 16 * (e & 3);
        if (r * TS + i >= n || c * TS + j >= n) continue;
#pragma unroll 1
        for (int l = 0; l < d; ++l) Js[l][tid] = sobol_J<KERN>(xr[i][l], xc[j][l], cst[l]);
        // the weight of the element: ONE place (a matrix entry can take the product's place)
        double wgt = twice * (wr[i] * wc[j]);
        if constexpr (MAT) wgt *= qs[i * (TS + 1) + j];
        double J[DD], A[DD];
#pragma unroll
        for (int l = 0; l < DD; ++l) {
            J[l] = Js[l][tid];
            A[l] = ar[i][l] * ac[j][l];
        }
        const double m0 = sobol_subset_product<DD>(0u, J, A);
#pragma unroll
        for (int s = 0; s < SC; ++s)
            if (s < ns) acc[s] = fma(wgt, sobol_subset_diff<DD>(mk.m[s], J, A, m0), acc[s]);
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int s = 0; s < SC; ++s) {
        const double f = sobol_wave_sum(acc[s]);
        if (lane == 0) red[wave][s] = f;
    }
    __syncthreads();
    if (tid < SC)
        part[(((size_t)z * ntile + r) * ntile + c) * SC + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// launch 3 of the subset pass: sobol_reduce_kernel's scheme over the columns of one chunk.  out[pair, s0 + s] = the sum over
// the pair's tiles of part[pair, tile, s] in a fixed order (thread t adds tiles t, t + 256, ..., then a tree over the threads);
// rows of `out` are ld doubles apart.  grid (masks of the chunk, pairs of the launch); sc = the columns per tile in part.
__global__ __launch_bounds__(256) void sobol_subset_reduce_kernel(const double* __restrict__ part, int ntile, int sc, SobolPairs pr,
                                                                  double* __restrict__ out, size_t ld) {
    __shared__ double red[256];
    const int s = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
    const int k = pr.k[z], kp = pr.kp[z];
    double acc = 0.0;
    for (int t = tid; t < ntile * ntile; t += 256) {
        const int r = t / ntile, c = t - r * ntile;
        if (k == kp && c > r) continue;
        acc += part[((size_t)z * ntile * ntile + t) * sc + s];
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[(size_t)z * ld + s] = red[0];
}

inline size_t sobol_subset_part_doubles(int n, int d, int npairs) {
    const size_t ntile = (n + TS - 1) / TS;
    return (size_t)(npairs < SOBOL_BATCH ? npairs : SOBOL_BATCH) * ntile * ntile * sobol_subset_chunk(d);
}

// launches 2 and 3 for the nb <= SOBOL_BATCH pairs in pr and ALL nsub masks, a chunk at a time: out[pair, s] (nb rows of nsub)
template <int MAT, int DD>
int sobol_subset_launches_dd(hipStream_t st, int kern, int n, int d, const double* x, const double* w, const double* ell,
                             const double* box, const double* tab, const SobolPairs& pr, int nb, double* part, double* out,
                             const SobolQ& qm, const uint64_t* masks, int nsub) {
    constexpr int SC = sobol_subset_chunk(DD);
    const int ntile = (n + TS - 1) / TS;
    const dim3 grid(ntile, ntile, nb);
    for (int s0 = 0; s0 < nsub; s0 += SC) {
        const int ns = nsub - s0 < SC ? nsub - s0 : SC;
        SobolMasks<SC> mk;
        for (int s = 0; s < SC; ++s) mk.m[s] = s < ns ? (unsigned)masks[s0 + s] : 0u;
        for_kern(kern, [&](auto kn) {
            hipLaunchKernelGGL((sobol_subset_kernel<decltype(kn)::value, DD, MAT>), grid, dim3(256), 0, st, x, n, d, w, ell, box, tab,
                               pr, ntile, part, qm, mk, ns);
        });
        CHECK_LAUNCH("sobol_subset_kernel");
        hipLaunchKernelGGL(sobol_subset_reduce_kernel, dim3(ns, nb), dim3(256), 0, st, (const double*)part, ntile, SC, pr, out + s0,
                           (size_t)nsub);
        CHECK_LAUNCH("sobol_subset_reduce_kernel");
    }
    return 0;
}

template <int MAT>
int sobol_subset_launches(hipStream_t st, int kern, int n, int d, const double* x, const double* w, const double* ell,
                          const double* box, const double* tab, const SobolPairs& pr, int nb, double* part, double* out,
                          const SobolQ& qm, const uint64_t* masks, int nsub) {
    if (d <= 8) return sobol_subset_launches_dd<MAT, 8>(st, kern, n, d, x, w, ell, box, tab, pr, nb, part, out, qm, masks, nsub);
    return sobol_subset_launches_dd<MAT, 16>(st, kern, n, d, x, w, ell, box, tab, pr, nb, part, out, qm, masks, nsub);
}

// do_sobol_pairs for a list of masks: the table and the means once (they stay in the scratch: tab, then means), then the pairs
// in batches of SOBOL_BATCH, each over every chunk of masks.  out is npairs x nsub.
template <int MAT>
int do_sobol_subset_pairs(hipStream_t st, int kern, int n, int d, int q_all, const double* x, const double* w, const double* ell,
                          const double* box, const int* pairs, int npairs, const uint64_t* masks, int nsub, void* scratch,
                          double* out, SobolQ qm) {
    double* tab = (double*)scratch;
    double* means = tab + (size_t)q_all * d * n;
    double* part = means + q_all;
    for_kern(kern, [&](auto kn) {
        hipLaunchKernelGGL((sobol_table_kernel<decltype(kn)::value>), dim3(q_all), dim3(256), 0, st, x, n, d, w, ell, box, tab, means);
    });
    CHECK_LAUNCH("sobol_table_kernel");
    for (int p0 = 0; p0 < npairs; p0 += SOBOL_BATCH) {
        const int nb = npairs - p0 < SOBOL_BATCH ? npairs - p0 : SOBOL_BATCH;
        SobolPairs pr;
        for (int i = 0; i < SOBOL_BATCH; ++i) {
            pr.k[i] = i < nb ? pairs[2 * (p0 + i)] : 0;
            pr.kp[i] = i < nb ? pairs[2 * (p0 + i) + 1] : 0;
        }
        int rc = sobol_subset_launches<MAT>(st, kern, n, d, x, w, ell, box, tab, pr, nb, part, out + (size_t)p0 * nsub, qm, masks, nsub);
        if (rc) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The matrix-weighted pass on a conditioned view (lcgp_condition_sobol_matrix_pairs).  Over the N = n + m centres
// [x; xn] the view's covariance correction is c^2 times
//     [[D sr sr^T o A^-1, 0], [0, 0]] + P P^T,     P = [ -D sr o (W^T T_n^T) ; L_S^-T ]  (N x m),   T_n = L_S^-1 U_n
// (the block inverse of the augmented matrix with the Schur complement S of 4.13).  The caller's row vectors carry c sr_i on the
// training rows and c on the new ones, so the weight of an element is v_i v_i' (E[i, i'] + D A^-1[i, i'] [i, i' < n]) with
//     E = Pt^T Pt,     Pt = [ D (-T_n W) | L_S^-1 ]   (m x N; sr left to v).
// One component at a time: -T_n by OP_COND_U on a zeroed slab (R := the dense L_S^-1, K = mpad), (-T_n) W by OP_PRED_V, the
// transposition with the scaling by D and the L_S^-T block (cond_sobol_p_kernel), the lower tiles of E by OP_PRED_COV on a
// zeroed E with its -D_k read from a word holding -1, and ONE pair pass over the N x N plane (SOBOL_VIEW).
// ---------------------------------------------------------------------------------------------------
struct CondSobolLay {
    int N, Npad, npad, mpad;
    size_t off_tab, off_means, off_part, off_neg, off_T, off_G, off_P, off_E, total;       // bytes
};

// subset: the tile sums are those of one chunk of masks (lcgp_condition_sobol_matrix_subset_pairs), everything else the same
inline CondSobolLay cond_sobol_carve(int n, int d, int q, int m, bool subset = false) {
    CondSobolLay L;
    L.N = n + m;
    L.Npad = round_up(L.N, TS);
    L.npad = round_up(n, 2 * TS);
    L.mpad = cov_pad(m);
    const size_t dbl = sizeof(double);
    size_t o = 0;
    L.off_tab = o; o = align256(o + (size_t)q * d * L.N * dbl);
    L.off_means = o; o = align256(o + (size_t)q * dbl);
    L.off_part = o; o = align256(o + (subset ? sobol_subset_part_doubles(L.N, d, 1) : sobol_part_doubles(L.N, d, 1, 1)) * dbl);
    L.off_neg = o; o = align256(o + dbl);
    L.off_T = o; o = align256(o + (size_t)L.mpad * L.npad * dbl);
    L.off_G = o; o = align256(o + (size_t)L.mpad * L.npad * dbl);
    L.off_P = o; o = align256(o + (size_t)L.Npad * L.mpad * dbl);
    L.off_E = o; o = align256(o + (size_t)L.Npad * L.Npad * dbl);
    L.total = o;
    return L;
}

// P[i, a] (Npad x mpad, row-major) from G = (-T_n) W (mpad x npad) and the dense L_S^-1 (mpad x mpad): D G[a, i] for i < n,
// L_S^-1[a, i - n] for n <= i < n + m, zero for i >= n + m and for a >= m.  64 x 64 tiles through LDS: reads run along i, writes
// along a.  Block (0, 0) also leaves the -1 that OP_PRED_COV takes for its -D_k.
__global__ __launch_bounds__(256) void cond_sobol_p_kernel(const double* __restrict__ G, int npad, const double* __restrict__ Wi,
                                                           int mpad, int n, int m, const double* __restrict__ dk,
                                                           double* __restrict__ P, double* __restrict__ neg) {
    __shared__ double tile[TS][TS + 1];
    const int i0 = blockIdx.x * TS, a0 = blockIdx.y * TS, tid = threadIdx.x;
    const double D = *dk;
    for (int e = tid; e < TS * TS; e += 256) {
        const int a = a0 + (e >> 6), i = i0 + (e & 63);
        double v = 0.0;
        if (a < m) {
            if (i < n) v = D * G[(size_t)a * npad + i];
            else if (i < n + m) v = Wi[(size_t)a * mpad + (i - n)];
        }
        tile[e >> 6][e & 63] = v;
    }
    __syncthreads();
    for (int e = tid; e < TS * TS; e += 256) {
        const int i = i0 + (e >> 6), a = a0 + (e & 63);
        P[(size_t)i * mpad + a] = tile[e & 63][e >> 6];
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *neg = -1.0;
}

// masks: NULL = the 2 d + 1 subsets of 4.22 (rows of 2 d + 2 in out); else the nsub masks of 4.25 (rows of nsub): the same
// preparation of E, only the pair launches differ
int do_condition_sobol(hipStream_t st, const Ws& w, const double* theta, const void* state, int m, const double* xa,
                       const double* v, const double* ell, const double* box, const int* ks, int nks, void* scratch, double* out,
                       const uint64_t* masks = nullptr, int nsub = 0) {
    const CondLay L = cond_carve(LCGP_F64, w.n, w.q, m);
    const CondSobolLay S = cond_sobol_carve(w.n, w.d, w.q, m, masks != nullptr);
    const int N = S.N, Npad = S.Npad, mpad = S.mpad, npad = w.npad, d = w.d, tw = w.d + 3 + w.p;
    char* sc = (char*)scratch;
    double* tab = (double*)(sc + S.off_tab);
    double* means = (double*)(sc + S.off_means);
    double* part = (double*)(sc + S.off_part);
    double* neg = (double*)(sc + S.off_neg);
    double* Tn = (double*)(sc + S.off_T);
    double* Gm = (double*)(sc + S.off_G);
    double* Pm = (double*)(sc + S.off_P);
    double* Em = (double*)(sc + S.off_E);
    for_kern(w.kern, [&](auto kn) {
        hipLaunchKernelGGL((sobol_table_kernel<decltype(kn)::value>), dim3(w.q), dim3(256), 0, st, xa, N, d, v, ell, box, tab, means);
    });
    CHECK_LAUNCH("sobol_table_kernel");
    const size_t slab = (size_t)mpad * npad;
    for (int r = 0; r < nks; ++r) {
        const int k = ks[r];
        const double* Un = (const double*)((const char*)state + L.off_U) + (size_t)k * slab;
        const double* Wi = (const double*)((const char*)state + L.off_W) + (size_t)k * mpad * mpad;
        const double* Wk = (const double*)(w.base + w.off_W) + (size_t)k * w.mat;
        const double* dk = theta + (size_t)k * tw + d + 2;
        hipError_t e = hipMemsetAsync(Tn, 0, slab * sizeof(double), st);
        if (e != hipSuccess) return fail("hipMemsetAsync", e);
        GemmArgs g;                                        // -T_n = 0 - L_S^-1 U_n
        g.A = Wi; g.B = Un; g.C = Tn;
        g.sA = (size_t)mpad * mpad; g.sB = g.sC = slab; g.ldA = mpad; g.ldB = g.ldC = npad;
        g.nb = w.nb; g.p0 = mpad / TS; g.p1 = mpad / TS; g.p2 = g.p3 = 0;
        int rc = launch_gemm<double, OP_COND_U, 64>(st, g, g.p0 * g.nb, 1);
        if (rc) return rc;
        rc = launch_pred<double, OP_PRED_V>(st, Tn, Wk, Gm, slab, w.mat, npad, mpad, w.nb, 1, 0, true);       // (-T_n) W
        if (rc) return rc;
        hipLaunchKernelGGL(cond_sobol_p_kernel, dim3(Npad / TS, mpad / TS), dim3(256), 0, st, (const double*)Gm, npad, Wi, mpad,
                           w.n, m, dk, Pm, neg);
        CHECK_LAUNCH("cond_sobol_p_kernel");
        e = hipMemsetAsync(Em, 0, (size_t)Npad * Npad * sizeof(double), st);
        if (e != hipSuccess) return fail("hipMemsetAsync", e);
        GemmArgs h;                                        // E += P P^T on the lower tiles (alpha = -(-1))
        h.A = Pm; h.B = Pm; h.C = Em;
        h.sA = h.sB = (size_t)Npad * mpad; h.sC = (size_t)Npad * Npad; h.ldA = h.ldB = mpad; h.ldC = Npad;
        h.p1 = 0; h.p2 = 0; h.p3 = 0;
        h.theta = neg;
        const int t64 = Npad / TS;
        h.nb = t64; h.p0 = mpad / TS;
        rc = launch_gemm<double, OP_PRED_COV, 64>(st, h, t64 * (t64 + 1) / 2, 1);
        if (rc) return rc;
        SobolPairs pr;
        for (int i = 0; i < SOBOL_BATCH; ++i) pr.k[i] = pr.kp[i] = k;
        SobolQ qm{(const double*)(w.base + w.off_V), w.mat, npad};
        qm.e = Em; qm.epad = Npad; qm.nt = w.n; qm.dk = dk;
        if (masks)
            rc = sobol_subset_launches<SOBOL_VIEW>(st, w.kern, N, d, xa, v, ell, box, tab, pr, 1, part, out + (size_t)r * nsub, qm,
                                                   masks, nsub);
        else
            rc = sobol_pair_launches<SOBOL_VIEW>(st, w.kern, N, d, xa, v, ell, box, tab, means, pr, 1, part,
                                                 out + (size_t)r * (2 * d + 2), qm);
        if (rc) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Exact box ALC (lcgp_hip.h: lcgp_box_alc; no counterpart in the reference): how much the box-integrated
// posterior variance IV_k of 4.23 drops if the simulator ran r more times at a candidate.  With c = scale (1 - nt), X_c the
// candidate's cross row (nugget entry at `match`), V_c = X_c A^-1, b_c = D c sr o V_c, J_l the pair average of sobol_J with both
// length scales equal, M[i, i'] = prod_l J_l(x_il, x_i'l), m_c[i] = prod_l J_l(x_cl, x_il), m_cc = prod_l J_l(x_cl, x_cl):
//     R(c) = [ c^2 m_cc - 2 c b_c . m_c + b_c^T M b_c ] / (max(scale - D |U_c|^2, 0) + 1 / (D r))
// The three terms cancel to a few parts in 1e5 of each: errors are stated against their absolute sum, never against R.
// Ms = (sr sr^T) o M is materialised once per group of components (box_matrix_kernel), X, U, gvar and V come from the launches of
// lcgp_predict_grad, T = V Ms from the tile kernel (OP_HESS_G) and T_c . V_c from pgrad_rowdot_kernel; box_cross_kernel sweeps the
// candidate's row for sum_i sr_i V_ci m_c[i] and combines.  Every row of every product depends on its candidate only and every sum
// has a fixed order: bitwise independent of the chunking, of the grouping and of the scratch content.
// ---------------------------------------------------------------------------------------------------
struct BoxLay {
    int npad, nb, n0p, n0r;
    size_t mat, slab;
    size_t off_m, off_x, off_u, off_gh, off_gv, off_rd, total;
};

// Ms first: its place does not depend on n_cand, so that the passes over the chunks of one candidate set share it
inline BoxLay box_carve(int n, int qg, int n0) {
    BoxLay L;
    L.npad = round_up(n, 2 * TS);
    L.nb = L.npad / TS;
    L.n0p = predict_pad(n0);                // rows of X / U / V the launches of lcgp_predict form
    L.n0r = round_up(n0, 2 * TS);           // rows of a slab: V Ms runs on 128 x 128 tiles
    L.mat = (size_t)L.npad * L.npad;
    L.slab = (size_t)L.n0r * L.npad;
    size_t o = 0;
    const size_t e = sizeof(double);
    L.off_m = o; o = align256(o + (size_t)qg * L.mat * e);
    L.off_x = o; o = align256(o + (size_t)qg * L.slab * e);
    L.off_u = o; o = align256(o + (size_t)qg * L.slab * e);
    L.off_gh = o; o = align256(o + (size_t)qg * L.n0r * e);
    L.off_gv = o; o = align256(o + (size_t)qg * L.n0r * e);
    L.off_rd = o; o = align256(o + (size_t)qg * L.n0r * e);
    L.total = o;
    return L;
}

// Ms_k = (sr sr^T) o M_k as a full npad x npad matrix, zero on the padding: one 64 x 64 tile (r, c), c <= r, per workgroup, 16
// elements per thread one after the other (a rolled loop over d around sobol_J: the code of one J is long), through LDS to the
// tile and to its mirror, both written in whole rows.  In a diagonal tile only j <= i is evaluated.
template <int KERN>
__global__ __launch_bounds__(256) void box_matrix_kernel(double* __restrict__ Ms, size_t mat, int n, int npad, int d,
                                                         const double* __restrict__ x, const double* __restrict__ sr,
                                                         const double* __restrict__ theta, int tw, const double* __restrict__ box) {
    __shared__ double tl[TS][TS + 1];
    __shared__ SobolDim cst[DWIDE];
    const int r = blockIdx.x, c = blockIdx.y, k = blockIdx.z;
    if (c > r) return;
    const int tid = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    if (tid < d) cst[tid] = sobol_dim<KERN>(th[tid], th[tid], box[tid], box[d + tid]);
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int i = ty * 4 + (e >> 2), j = tx + 16 * (e & 3);
        const int gi = r * TS + i, gj = c * TS + j;
        if (r == c && j > i) continue;
        double v = 0.0;
        if (gi < n && gj < n) {
            const double* xi = x + (size_t)gi * d;
            const double* xj = x + (size_t)gj * d;
            v = sr ? sr[gi] * sr[gj] : 1.0;
#pragma unroll 1
            for (int l = 0; l < d; ++l) v *= sobol_J<KERN>(xi[l], xj[l], cst[l]);
        }
        tl[i][j] = v;
    }
    __syncthreads();
    double* Mk = Ms + (size_t)k * mat;
    for (int e = tid; e < TS * TS; e += 256) {
        const int i = e >> 6, j = e & 63;
        if (r == c) {
            Mk[(size_t)(r * TS + i) * npad + c * TS + j] = j <= i ? tl[i][j] : tl[j][i];
        } else {
            Mk[(size_t)(r * TS + i) * npad + c * TS + j] = tl[i][j];
            Mk[(size_t)(c * TS + i) * npad + r * TS + j] = tl[j][i];
        }
    }
}

// One workgroup per (candidate, component): s1 = sum_i sr_i V[c, i] m_c[i] over the row (m_c[i] a rolled loop over d around
// sobol_J, nothing of size n_cand x n reaches memory; butterflies inside a wave, then the four waves in order), m_cc, and with
// rd = T_c . V_c (pgrad_rowdot_kernel) and gvar (pred_reduce_kernel) the score
//     R = c^2 [ m_cc - 2 D s1 + D^2 rd ] / (max(gvar, 0) + 1 / (D r))
// into out[k, c].  Not clamped: a gain at rounding level may come out slightly negative.
template <int KERN>
__global__ __launch_bounds__(256) void box_cross_kernel(const double* __restrict__ x0, const double* __restrict__ x,
                                                        const double* __restrict__ sr, int n, int npad, int d,
                                                        const double* __restrict__ theta, int tw, const double* __restrict__ box,
                                                        const double* __restrict__ V, size_t slab, const double* __restrict__ rd,
                                                        const double* __restrict__ gvar, int n0r, int nrep, int ldo,
                                                        double* __restrict__ out) {
    __shared__ double x0l[DWIDE];
    __shared__ SobolDim cst[DWIDE];
    __shared__ double sh[4];
    const int i0 = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const double* th = theta + (size_t)k * tw;
    if (tid < d) {
        x0l[tid] = x0[(size_t)i0 * d + tid];
        cst[tid] = sobol_dim<KERN>(th[tid], th[tid], box[tid], box[d + tid]);
    }
    __syncthreads();
    const double* vr = V + (size_t)k * slab + (size_t)i0 * npad;
    double acc = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double* xi = x + (size_t)i * d;
        double m = sr ? sr[i] : 1.0;
#pragma unroll 1
        for (int l = 0; l < d; ++l) m *= sobol_J<KERN>(x0l[l], xi[l], cst[l]);
        acc = fma(vr[i], m, acc);
    }
    const double s1 = hess_block_sum(acc, sh, tid);
    if (tid != 0) return;
    double mcc = 1.0;
#pragma unroll 1
    for (int l = 0; l < d; ++l) mcc *= sobol_J<KERN>(x0l[l], x0l[l], cst[l]);
    const double scale = th[d], nug = th[d + 1], D = th[d + 2];
    const double cc = scale / (1.0 + nug);                // scale (1 - nt)
    const double t0 = cc * cc * mcc, t1 = 2.0 * cc * (D * cc * s1), t2 = (D * cc) * (D * cc) * rd[(size_t)k * n0r + i0];
    const double den = fmax(gvar[(size_t)k * n0r + i0], 0.0) + 1.0 / (D * (double)nrep);
    out[(size_t)k * ldo + i0] = ((t0 - t1) + t2) / den;
}

// enqueues the pass for the components [k0, k0 + qg) of the workspace and n0 candidates; form_m = 0: Ms of these components is
// still in the scratch from the preceding call (same k0, qg, box)
int do_box_alc(hipStream_t st, const Ws& w, const void* x, const void* sr, const double* theta, int k0, int qg, const double* box,
               int n0, const void* x0, const int* match, int nrep, int form_m, char* scratch, double* out, int ldo) {
    const int n = w.n, d = w.d, npad = w.npad, tw = d + 3 + w.p;
    const BoxLay L = box_carve(n, qg, n0);
    double* Ms = (double*)(scratch + L.off_m);
    double* X = (double*)(scratch + L.off_x);          // X, then V
    double* U = (double*)(scratch + L.off_u);          // U, then T
    double* GH = (double*)(scratch + L.off_gh);
    double* GV = (double*)(scratch + L.off_gv);
    double* RD = (double*)(scratch + L.off_rd);
    const double* W = (const double*)(w.base + w.off_W) + (size_t)k0 * w.mat;
    const double* zv = (const double*)(w.base + w.off_z) + (size_t)k0 * npad;
    const double* th = theta + (size_t)k0 * tw;
    const double* xd = (const double*)x;
    const double* srd = (const double*)sr;
    const double* x0d = (const double*)x0;
    if (form_m) {
        for_kern(w.kern, [&](auto kern) {
            hipLaunchKernelGGL((box_matrix_kernel<decltype(kern)::value>), dim3(w.nb, w.nb, qg), dim3(256), 0, st, Ms, L.mat, n, npad,
                               d, xd, srd, th, tw, box);
        });
        CHECK_LAUNCH("box_matrix_kernel");
    }
    // X (nugget entry at match), U = X W^T, gvar, V = U W: the launches of lcgp_predict_grad on the group's components
    ThetaArg dummy;
    memset(&dummy, 0, sizeof(dummy));
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((cross_kernel<double, decltype(kern)::value>), dim3(w.nb, L.n0p / TS, qg), dim3(256), 0, st, X, npad, n0, n, d,
                           x0d, xd, dummy, th, 0, srd, L.n0p, npad, tw, L.slab, match);
    });
    CHECK_LAUNCH("cross_kernel");
    int rc = launch_pred<double, OP_PRED_U>(st, X, W, U, L.slab, w.mat, npad, L.n0p, w.nb, qg);
    if (rc) return rc;
    hipLaunchKernelGGL((pred_reduce_kernel<double>), dim3(n0, qg), dim3(64), 0, st, (const double*)X, (const double*)U, L.slab, L.slab,
                       npad, n, zv, npad, th, tw, d, L.n0r, GH, GV);
    CHECK_LAUNCH("pred_reduce_kernel");
    // OP_PRED_V sums in another order on 128-row tiles: below 128 candidates 64-row tiles whatever the padding,
    // from 128 on the caller never passes fewer, so that a row's V does not depend on the chunking
    rc = launch_pred<double, OP_PRED_V>(st, U, W, X, L.slab, w.mat, npad, L.n0p, w.nb, qg, 0, n0 < 2 * TS);
    if (rc) return rc;
    const double* V = X;
    // T = V Ms (rows beyond n0p of a slab are never written: their products are never read), then T_c . V_c
    GemmArgs g;
    g.A = V; g.B = Ms; g.C = U; g.ldA = g.ldB = g.ldC = npad;
    g.sA = L.slab; g.sB = L.mat; g.sC = L.slab;
    g.nb = L.nb / 2; g.p0 = L.n0r / (2 * TS); g.p1 = L.nb / 2; g.p2 = g.p3 = 0;
    rc = launch_gemm<double, OP_HESS_G, 128>(st, g, g.p0 * g.nb, qg);
    if (rc) return rc;
    hipLaunchKernelGGL(pgrad_rowdot_kernel, dim3(n0, qg), dim3(64), 0, st, (const double*)U, V, L.slab, npad, n, RD, (size_t)L.n0r);
    CHECK_LAUNCH("pgrad_rowdot_kernel");
    for_kern(w.kern, [&](auto kern) {
        hipLaunchKernelGGL((box_cross_kernel<decltype(kern)::value>), dim3(n0, qg), dim3(256), 0, st, x0d, xd, srd, n, npad, d, th, tw,
                           box, V, L.slab, (const double*)RD, (const double*)GV, L.n0r, nrep, ldo, out + (size_t)k0 * ldo);
    });
    CHECK_LAUNCH("box_cross_kernel");
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
#ifndef LCGP_SRC_HASH
#define LCGP_SRC_HASH "unknown"
#endif

namespace {

// ---- what the entries share ("Writing an entry": how an entry and its twin on a conditioned view are written) ----
// opens an entry: check_common, then the carved workspace with its kernel and the stream (nothing is read or enqueued)
int open_entry(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* workspace, Ws& w,
               hipStream_t& st) {
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    w = carve(dtype, n, d, p, q_local, (void*)workspace);
    w.kern = kernel_id;
    st = (hipStream_t)stream;
    return 0;
}

// f(double{}) or f(float{}): the one place a dtype becomes a template argument (f: a generic lambda calling do_x<decltype(t)>)
template <typename F>
int by_dtype(int dtype, F&& f) {
    return dtype == LCGP_F64 ? f(double{}) : f(float{});
}

// the conditioned view a twin entry runs on (a null ViewArg*: the fitted model) and the size of the caller's scratch, which
// only the view entries are told and test last
struct ViewArg {
    const void* state;
    int m;
    const void* xn;
    const void* grad_state;
    size_t scratch_bytes;
};

int check_view(int m) {
    if (m < 1) return bad("m < 1");
    return 0;
}

VrView view_of(int dtype, int n, int q_local, const ViewArg& v) {
    const CondLay L = cond_carve(dtype, n, q_local, v.m);
    VrView cv;
    cv.Un = (const char*)v.state + L.off_U; cv.Wi = (const char*)v.state + L.off_W; cv.xn = v.xn;
    cv.m = v.m; cv.mpad = L.mpad;
    return cv;
}

// match_host / match go together; the host copy is scanned here (n_cand entries: -1 or a training index)
int check_match(int n, int n_cand, const int* match_host, const int* match) {
    if ((match_host == nullptr) != (match == nullptr)) return bad("match_host and match must both be NULL or both be given");
    if (match_host)
        for (int i = 0; i < n_cand; ++i)
            if (match_host[i] < -1 || match_host[i] >= n) return bad("match must be -1 or a training index in [0, n)");
    return 0;
}

// ---- the per-point queries: lcgp_predict, lcgp_predict_grad, lcgp_predict_hess, lcgp_predict_gradcov and their twins ----
enum PointKind { PT_VALUE, PT_GRAD, PT_HESS, PT_GRADCOV };

// o: the entry's output pointers in its own order (PT_GRADCOV: dghat, gamma, M; wt its weights); same: lcgp_predict only
int point_checked(PointKind kind, void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                  const void* sr, const double* theta, const void* workspace, const ViewArg* v, int n0, const void* x0, int same,
                  void* scratch, double* const (&o)[6], const double* wt, int out_stride) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (v && (rc = check_view(v->m))) return rc;
    if (n0 < 1) return bad("n0 < 1");
    if (kind >= PT_HESS && (long long)n0 * d > LCGP_HESS_MAX_ROWS)
        return bad("n0 * d must be <= LCGP_HESS_MAX_ROWS: pass the new inputs in chunks");
    bool null = !x || !theta || !workspace || !x0 || !scratch;
    if (v) null = null || !v->state || !v->xn || (kind != PT_VALUE && !v->grad_state);
    for (int i = 0; i < (kind == PT_GRADCOV ? 1 : 2 * (kind + 1)); ++i) null = null || !o[i];
    if (null) return bad("NULL pointer");
    if (kind == PT_GRADCOV) {
        if (!o[1] && !wt) return bad("NULL pointer: gamma may only be NULL when w is given");
        if ((wt != nullptr) != (o[2] != nullptr)) return bad("w and M go together: both or neither");
    }
    if (out_stride != 0 && out_stride < n0) return bad("out_stride must be 0 (= n0) or >= n0");
    if (v) {
        static const char* const small[] = {
            "scratch is smaller than lcgp_condition_scratch_bytes(dtype, n, q_local, m, n0)",
            "scratch is smaller than lcgp_condition_predict_grad_scratch_bytes(dtype, n, q_local, m, n0)",
            "scratch is smaller than lcgp_condition_predict_hess_scratch_bytes(dtype, n, d, q_local, m, n0)",
            "scratch is smaller than lcgp_condition_predict_gradcov_scratch_bytes(dtype, n, d, q_local, m, n0)"};
        const size_t need = (kind != PT_GRADCOV ? cond_predict_scratch(dtype, n, q_local, v->m, n0) : 0) +
                            (kind >= PT_HESS ? cond_rows_scratch(dtype, n, d, q_local, v->m, n0) : 0);
        if (v->scratch_bytes < need) return bad(small[kind]);
    }
    const int ldo = out_stride ? out_stride : n0;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (kind == PT_VALUE)
            return v ? do_condition_predict<T>(st, w, x, sr, theta, v->state, v->m, v->xn, n0, x0, scratch, o[0], o[1], ldo)
                     : do_predict<T>(st, w, x, sr, theta, n0, x0, same, scratch, o[0], o[1], ldo);
        if (kind == PT_GRAD)
            return v ? do_condition_predict_grad<T>(st, w, x, sr, theta, v->state, v->m, v->xn, v->grad_state, n0, x0, scratch, o[0],
                                                    o[1], o[2], o[3], ldo)
                     : do_predict_grad<T>(st, w, x, sr, theta, n0, x0, scratch, o[0], o[1], o[2], o[3], ldo);
        if (kind == PT_HESS)
            return v ? do_condition_predict_hess<T>(st, w, x, sr, theta, v->state, v->m, v->xn, v->grad_state, n0, x0, scratch, o[0],
                                                    o[1], o[2], o[3], o[4], o[5], ldo)
                     : do_predict_hess<T>(st, w, x, sr, theta, n0, x0, scratch, o[0], o[1], o[2], o[3], o[4], o[5], ldo);
        return v ? do_condition_predict_gradcov<T>(st, w, x, sr, theta, v->state, v->m, v->xn, v->grad_state, n0, x0, scratch, o[0],
                                                   o[1], wt, o[2], ldo)
                 : do_predict_gradcov<T>(st, w, x, sr, theta, n0, x0, scratch, o[0], o[1], wt, o[2], ldo);
    });
}

// lcgp_predict_hess_scratch_bytes / lcgp_predict_gradcov_scratch_bytes and their twins (m: the view's new inputs)
int rows_bytes(bool hess, int dtype, int n, int d, int q_local, const int* m, int n0, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (m ? (n < 1 || q_local < 1) : (n < 1 || n0 < 1 || q_local < 1))
        return bad(m ? "n, q_local must be >= 1" : "n, n0, q_local must be >= 1");
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (m && *m < 1) return bad("m < 1");
    if (m && n0 < 1) return bad("n0 < 1");
    if ((long long)n0 * d > LCGP_HESS_MAX_ROWS) return bad("n0 * d must be <= LCGP_HESS_MAX_ROWS: pass the new inputs in chunks");
    if (!bytes) return bad("bytes is NULL");
    if (m)
        *bytes = (hess ? cond_predict_scratch(dtype, n, q_local, *m, n0) : 0) + cond_rows_scratch(dtype, n, d, q_local, *m, n0);
    else
        *bytes = 2 * (size_t)q_local * ((hess ? predict_pad(n0) : 0) + (size_t)hess_rows_pad(n0, d)) * round_up(n, 2 * TS) *
                 (dtype == LCGP_F64 ? 8 : 4);
    return 0;
}

// ---- lcgp_predict_cov and its twin ----
int cov_checked(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                const double* theta, const void* workspace, const ViewArg* v, int n0, const void* x0, int same, void* scratch,
                void* cov_workspace, double jitter) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (v && (rc = check_view(v->m))) return rc;
    if (n0 < 1) return bad("n0 < 1");
    if (!v && (same < 0 || (same > 0 && same - 1 + n0 > n))) return bad("same must be 0 or 1 + the row offset of x0 within x");
    if (!(jitter >= 0.0) || !__builtin_isfinite(jitter)) return bad("jitter must be finite and >= 0");
    if (!x || !theta || !workspace || (v && (!v->state || !v->xn)) || !x0 || !scratch || !cov_workspace) return bad("NULL pointer");
    if (v && v->scratch_bytes < cond_cov_carve(dtype, n, q_local, v->m, n0).total)
        return bad("scratch is smaller than lcgp_condition_predict_cov_scratch_bytes(dtype, n, q_local, m, n0)");
    const Ws cw = carve(dtype, n0, d, p, q_local, cov_workspace);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return v ? do_condition_predict_cov<T>(st, w, x, sr, theta, view_of(dtype, n, q_local, *v), n0, x0, (char*)scratch, cw, jitter)
                 : do_predict_cov<T>(st, w, x, sr, theta, n0, x0, same, scratch, cw, jitter);
    });
}

// ---- lcgp_predict_marginal (v == nullptr) and lcgp_condition_predict_marginal, which also runs without a state (m == 0) ----
int marginal_checked(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                     const double* theta, const void* workspace, const ViewArg* v, int n0, const void* x0,
                     const unsigned char* mask, const double* box, void* scratch, double* ghat, double* gvar, int out_stride,
                     const MargRef& ref) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (v && (v->state ? v->m < 1 : v->m != 0)) return bad("m must be >= 1 with a state and 0 without one");
    if (n0 < 1) return bad("n0 < 1");
    if (!x || !theta || !workspace || !x0 || !mask || !box || !scratch || !ghat || !gvar) return bad("NULL pointer");
    if (v && v->state && !v->xn) return bad("NULL pointer");
    if (ref.out && (ref.row < 0 || ref.row >= n0)) return bad("ref_row must be a row of the pass");
    if (ref.in && (!ref.x || !ref.mask || !ref.gcov)) return bad("ref_in needs ref_x, ref_mask and gcov");
    if (out_stride != 0 && out_stride < n0) return bad("out_stride must be 0 (= n0) or >= n0");
    if (v) {
        size_t need = 0;
        if ((rc = lcgp_condition_predict_marginal_scratch_bytes(dtype, n, d, q_local, v->m, n0, &need))) return rc;
        if (v->scratch_bytes < need)
            return bad("scratch is smaller than lcgp_condition_predict_marginal_scratch_bytes(dtype, n, d, q_local, m, n0)");
    }
    const int ldo = out_stride ? out_stride : n0;
    return by_dtype(dtype, [&](auto t) {
        return do_predict_marginal<decltype(t)>(st, w, x, sr, theta, v ? v->state : nullptr, v ? v->m : 0, v ? v->xn : nullptr, n0, x0,
                                                mask, box, scratch, ghat, gvar, ldo, ref);
    });
}

}  // namespace

extern "C" {

int lcgp_version(void) { return LCGP_VERSION; }
const char* lcgp_source_hash(void) { return LCGP_SRC_HASH; }
const char* lcgp_last_error(void) { return g_err; }
int lcgp_theta_width(int d, int p) { return d + 3 + p; }
int lcgp_out_width(int d, int p) { return d + 5 + p; }
int lcgp_partial_width(int d, int p, int q_total) { return 3 + q_total * d + 2 * q_total + p; }

int lcgp_sched_default(lcgp_sched* sched) {
    if (!sched) return bad("sched is NULL");
    *sched = default_sched();
    return 0;
}

int lcgp_workspace_bytes(int dtype, int n, int d, int p, int q_local, size_t* bytes) {
    int rc = check_common(dtype, n, d, p, q_local);
    if (rc) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = carve(dtype, n, d, p, q_local, nullptr).total;
    return 0;
}

int lcgp_predict_scratch_bytes(int dtype, int n, int q_local, int n0, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || n0 < 1 || q_local < 1) return bad("n, n0, q_local must be >= 1");
    if (!bytes) return bad("bytes is NULL");
    const size_t npad = round_up(n, 2 * TS), n0pad = predict_pad(n0);
    *bytes = 2 * (size_t)q_local * n0pad * npad * (dtype == LCGP_F64 ? 8 : 4);
    return 0;
}

int lcgp_covmat(void* stream, int dtype, int kernel_id, int n1, int n2, int d, const void* x1, const void* x2, const double* ell,
                double scale, double nug, int same, void* out) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (kernel_id != LCGP_KERNEL_MATERN32 && kernel_id != LCGP_KERNEL_SE && kernel_id != LCGP_KERNEL_MATERN52)
        return bad("kernel_id must be 0 (Matern-3/2), 1 (squared exponential) or 2 (Matern-5/2)");
    if (n1 < 1 || n2 < 1) return bad("n1/n2 < 1");
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (!x1 || !x2 || !ell || !out) return bad("NULL pointer");
    ThetaArg th;
    memset(&th, 0, sizeof(th));
    for (int j = 0; j < d; ++j) th.v[j] = ell[j];
    th.v[d] = scale;
    th.v[d + 1] = nug;
    return by_dtype(dtype, [&](auto t) { return do_matern<decltype(t)>((hipStream_t)stream, kernel_id, n1, n2, d, x1, x2, th, same, out); });
}
int lcgp_matern32(void* stream, int dtype, int n1, int n2, int d, const void* x1, const void* x2, const double* ell,
                  double scale, double nug, int same, void* out) {
    return lcgp_covmat(stream, dtype, LCGP_KERNEL_MATERN32, n1, n2, d, x1, x2, ell, scale, nug, same, out);
}

int lcgp_kernel_build(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                      const double* theta, void* workspace) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (!x || !theta || !workspace) return bad("NULL pointer");
    return by_dtype(dtype, [&](auto t) { return do_build<decltype(t)>(st, w, x, sr, theta); });
}

int lcgp_potrf_logdet(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace, double* half_logdet,
                      int* info, const lcgp_sched* sched, const void* plan) {
    const void* plan_host = plan;
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (!workspace) return bad("NULL workspace");
    lcgp_sched sc;
    if ((rc = resolve_sched(sched, sc))) return rc;
    if (plan_host && (rc = check_plan(plan_host, dtype, n, q_local, false))) return rc;
    rc = by_dtype(dtype, [&](auto t) { return do_potrf<decltype(t)>(st, w, sc, false, false, nullptr, plan_host); });
    if (rc) return rc;
    if (half_logdet || info) {
        hipLaunchKernelGGL(copy_stats_kernel, dim3((q_local + 63) / 64), dim3(64), 0, st,
                           (const double*)(w.base + w.off_logdet), (const int*)(w.base + w.off_info), half_logdet, info,
                           q_local);
        CHECK_LAUNCH("copy_stats");
    }
    return 0;
}

// lcgp_potri (stage 0), lcgp_trtri (1), lcgp_lauum (2)
static int inverse_stage(int stage, void* stream, int dtype, int n, int d, int p, int q_local, void* workspace,
                         const lcgp_sched* sched) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (!workspace) return bad("NULL workspace");
    lcgp_sched sc;
    if ((rc = resolve_sched(sched, sc))) return rc;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return stage == 0 ? do_potri<T>(st, w, sc) : stage == 1 ? do_trtri<T>(st, w, sc) : do_lauum<T>(st, w, sc);
    });
}

int lcgp_potri(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace, const lcgp_sched* sched) {
    return inverse_stage(0, stream, dtype, n, d, p, q_local, workspace, sched);
}
int lcgp_trtri(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace, const lcgp_sched* sched) {
    return inverse_stage(1, stream, dtype, n, d, p, q_local, workspace, sched);
}
int lcgp_lauum(void* stream, int dtype, int n, int d, int p, int q_local, void* workspace, const lcgp_sched* sched) {
    return inverse_stage(2, stream, dtype, n, d, p, q_local, workspace, sched);
}

int lcgp_lauum_clock(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace,
                     unsigned long long* out) {
    int rc = check_common(dtype, n, d, p, q_local);
    if (rc) return rc;
    if (!workspace || !out) return bad("NULL pointer");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    hipError_t e = hipMemcpyAsync(out, w.base + w.off_clock, 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return fail("hipMemcpyAsync", e);
    // read and clear: a second read without a stamped launch in between returns zeros (the 64x64-tile form of the launch,
    // which small problems and single components use, does not stamp), and so does a read after one call on a fresh workspace
    e = hipMemsetAsync(w.base + w.off_clock, 0, 2 * sizeof(unsigned long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail("hipMemsetAsync", e);
    return 0;
}

int lcgp_fetch_matrix(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace, int which, int k,
                      void* out) {
    int rc = check_common(dtype, n, d, p, q_local);
    if (rc) return rc;
    if (!workspace || !out) return bad("NULL pointer");
    if (which < 0 || which > 2 || k < 0 || k >= q_local) return bad("which/k out of range");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    size_t off = which == 0 ? w.off_M : (which == 1 ? w.off_W : w.off_V);
    dim3 grid((n + 255) / 256, n);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LCGP_F64)
        hipLaunchKernelGGL((fetch_kernel<double>), grid, dim3(256), 0, st,
                           (const double*)(w.base + off) + (size_t)k * w.mat, w.npad, n, (double*)out);
    else
        hipLaunchKernelGGL((fetch_kernel<float>), grid, dim3(256), 0, st,
                           (const float*)(w.base + off) + (size_t)k * w.mat, w.npad, n, (float*)out);
    CHECK_LAUNCH("fetch_kernel");
    return 0;
}

int lcgp_fetch_vector(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace, int which, int k,
                      void* out) {
    int rc = check_common(dtype, n, d, p, q_local);
    if (rc) return rc;
    if (!workspace || !out) return bad("NULL pointer");
    if (which < 0 || which > 1 || k < 0 || k >= q_local) return bad("which/k out of range");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    const char* src = w.base + (which == 0 ? w.off_b : w.off_z) + (size_t)k * w.npad * w.esz;
    hipError_t e = hipMemcpyAsync(out, src, (size_t)n * w.esz, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return fail("hipMemcpyAsync", e);
    return 0;
}

int lcgp_nll_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* Y,
                  const void* sr, const double* theta, void* workspace, double* out, const lcgp_sched* sched,
                  const void* plan) {
    const void* plan_host = plan;
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (!x || !Y || !theta || !workspace || !out) return bad("NULL pointer");
    lcgp_sched sc;
    if (plan_host) {
        // the plan carries the schedule it was built for (the stages behind the factorisation read their thresholds there)
        if ((rc = check_plan(plan_host, dtype, n, q_local, true))) return rc;
        sc = ((const PlanHeader*)plan_host)->sched;
    } else if ((rc = resolve_sched(sched, sc))) {
        return rc;
    }
    return by_dtype(dtype, [&](auto t) { return do_nll_grad<decltype(t)>(st, w, sc, x, Y, sr, theta, out, plan_host); });
}

int lcgp_nll_hess_width(int d, int p) { return hess_out_width(d, p); }

static int check_nll_hess(int dtype) {
    if (dtype == LCGP_F32) return bad("lcgp_nll_hess is float64 only (the trace difference of the kernel block cancels heavily): "
                                      "evaluate on a float64 workspace");
    return 0;
}

int lcgp_nll_hess_scratch_bytes(int dtype, int n, int d, int p, int q_group, size_t* bytes) {
    int rc = check_common(dtype, n, d, p, q_group);
    if (rc) return rc;
    if ((rc = check_nll_hess(dtype))) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = hess_carve(n, d, p, q_group).total;
    return 0;
}

int lcgp_nll_hess(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* Y,
                  const void* sr, const double* theta, const void* workspace, int k0, int q_group, void* scratch, double* out) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if ((rc = check_nll_hess(dtype))) return rc;
    if (k0 < 0 || q_group < 1 || k0 + q_group > q_local) return bad("k0 / q_group must select components inside [0, q_local)");
    if (!x || !Y || !theta || !workspace || !scratch || !out) return bad("NULL pointer");
    return do_nll_hess(st, w, x, (const double*)Y, sr, theta, k0, q_group, (char*)scratch, out);
}

static int check_predict_paramgrad(int dtype, int n0) {
    if (dtype == LCGP_F32) return bad("lcgp_predict_paramgrad is float64 only (the variance derivatives are differences that cancel): "
                                      "evaluate on a float64 workspace");
    if (n0 < 1 || n0 > 65535) return bad("n0 must be in [1, 65535]: pass the new inputs in chunks");
    return 0;
}

int lcgp_predict_paramgrad_scratch_bytes(int dtype, int n, int d, int p, int q_group, int n0, size_t* bytes) {
    int rc = check_common(dtype, n, d, p, q_group);
    if (rc) return rc;
    if ((rc = check_predict_paramgrad(dtype, n0))) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = pgrad_carve(n, d, p, q_group, n0).total;
    return 0;
}

int lcgp_predict_paramgrad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* Y,
                           const void* sr, const double* theta, const void* workspace, int k0, int q_group, int n0, const void* x0,
                           int same, void* scratch, double* ghat, double* gvar, double* dghat, double* dgvar, double* dghat_noise,
                           int out_stride) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if ((rc = check_predict_paramgrad(dtype, n0))) return rc;
    if (k0 < 0 || q_group < 1 || k0 + q_group > q_local) return bad("k0 / q_group must select components inside [0, q_local)");
    if (!x || !Y || !theta || !workspace || !x0 || !scratch || !ghat || !gvar || !dghat || !dgvar || !dghat_noise)
        return bad("NULL pointer");
    if (out_stride != 0 && out_stride < n0) return bad("out_stride must be 0 (= n0) or >= n0");
    if (same < 0 || (same > 0 && (long long)same - 1 + n0 > n)) return bad("same: the rows of x0 must be training inputs same - 1 .. same - 2 + n0");
    return do_predict_paramgrad(st, w, x, (const double*)Y, sr, theta, k0, q_group, n0, x0, same, (char*)scratch,
                                ghat, gvar, dghat, dgvar, dghat_noise, out_stride ? out_stride : n0);
}

int lcgp_plan_bytes(int dtype, int n, int q_local, int with_inverse, const lcgp_sched* sched, size_t* bytes) {
    int rc = check_common(dtype, n, 1, 1, q_local);
    if (rc) return rc;
    if (!bytes) return bad("bytes is NULL");
    lcgp_sched sc;
    if ((rc = resolve_sched(sched, sc))) return rc;
    *bytes = make_plan(dtype, n, q_local, with_inverse != 0, sc, nullptr);
    return *bytes ? 0 : -1;
}

int lcgp_plan_build(int dtype, int n, int q_local, int with_inverse, const lcgp_sched* sched, void* plan, size_t bytes) {
    int rc = check_common(dtype, n, 1, 1, q_local);
    if (rc) return rc;
    if (!plan) return bad("plan is NULL");
    lcgp_sched sc;
    if ((rc = resolve_sched(sched, sc))) return rc;
    const size_t need = make_plan(dtype, n, q_local, with_inverse != 0, sc, nullptr);
    if (!need) return -1;
    if (bytes < need) return bad("plan buffer too small (lcgp_plan_bytes)");
    return make_plan(dtype, n, q_local, with_inverse != 0, sc, plan) ? 0 : -1;
}

int lcgp_plan_info(const void* plan, int* nlaunch, int* inverse_done) {
    if (!plan) return bad("plan is NULL");
    const PlanHeader* h = (const PlanHeader*)plan;
    if (h->magic != PLAN_MAGIC || h->version != LCGP_VERSION) return bad("plan: not a plan of this library version");
    if (nlaunch) *nlaunch = h->nlaunch;
    if (inverse_done) *inverse_done = h->inverse_done;
    return 0;
}

int lcgp_pack_partial(void* stream, int d, int p, int q_local, int q_total, const int* comp, const double* theta,
                      const double* out, const double* guard, double* vec) {
    if (d < 1 || d > DWIDE || p < 1) return bad("d must be in [1, 126], p >= 1");
    if (q_local < 0 || q_total < 1 || q_local > q_total) return bad("need 0 <= q_local <= q_total, q_total >= 1");
    if (!vec || (q_local > 0 && (!comp || !theta || !out))) return bad("NULL pointer");
    hipLaunchKernelGGL(pack_partial_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d, p, q_local, q_total, comp, theta,
                       out, guard, vec);
    CHECK_LAUNCH("pack_partial_kernel");
    return 0;
}

int lcgp_predict(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                 const double* theta, const void* workspace, int n0, const void* x0, int same, void* scratch,
                 double* ghat, double* gvar, int out_stride) {
    double* const o[6] = {ghat, gvar};
    return point_checked(PT_VALUE, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n0, x0, same, scratch,
                         o, nullptr, out_stride);
}

int lcgp_predict_marginal_scratch_bytes(int dtype, int n, int d, int q_local, int n0, size_t* bytes) {
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    int rc = lcgp_predict_scratch_bytes(dtype, n, q_local, n0, bytes);
    if (rc) return rc;
    *bytes += (size_t)q_local * d * (round_up(n, 2 * TS) + 1) * sizeof(double);
    return 0;
}

int lcgp_predict_marginal(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                          const double* theta, const void* workspace, int n0, const void* x0, const unsigned char* mask,
                          const double* box, void* scratch, double* ghat, double* gvar, int out_stride) {
    return marginal_checked(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n0, x0, mask, box, scratch,
                            ghat, gvar, out_stride, MargRef());
}

int lcgp_predict_grad_scratch_bytes(int dtype, int n, int q_local, int n0, size_t* bytes) {
    return lcgp_predict_scratch_bytes(dtype, n, q_local, n0, bytes);
}

int lcgp_predict_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                      const double* theta, const void* workspace, int n0, const void* x0, void* scratch,
                      double* ghat, double* gvar, double* dghat, double* dgvar, int out_stride) {
    double* const o[6] = {ghat, gvar, dghat, dgvar};
    return point_checked(PT_GRAD, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n0, x0, 0, scratch, o,
                         nullptr, out_stride);
}

int lcgp_predict_hess_scratch_bytes(int dtype, int n, int d, int q_local, int n0, size_t* bytes) {
    return rows_bytes(true, dtype, n, d, q_local, nullptr, n0, bytes);
}

int lcgp_predict_hess(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                      const double* theta, const void* workspace, int n0, const void* x0, void* scratch,
                      double* ghat, double* gvar, double* dghat, double* dgvar, double* d2ghat, double* d2gvar, int out_stride) {
    double* const o[6] = {ghat, gvar, dghat, dgvar, d2ghat, d2gvar};
    return point_checked(PT_HESS, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n0, x0, 0, scratch, o,
                         nullptr, out_stride);
}

int lcgp_predict_gradcov_scratch_bytes(int dtype, int n, int d, int q_local, int n0, size_t* bytes) {
    return rows_bytes(false, dtype, n, d, q_local, nullptr, n0, bytes);
}

int lcgp_predict_gradcov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                         const double* theta, const void* workspace, int n0, const void* x0, void* scratch, double* dghat,
                         double* gamma, const double* w, double* M, int out_stride) {
    double* const o[6] = {dghat, gamma, M};
    return point_checked(PT_GRADCOV, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n0, x0, 0, scratch,
                         o, w, out_stride);
}

int lcgp_predict_cov_scratch_bytes(int dtype, int n, int q_local, int n0, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || n0 < 1 || q_local < 1) return bad("n, n0, q_local must be >= 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = 2 * (size_t)q_local * cov_pad(n0) * round_up(n, 2 * TS) * (dtype == LCGP_F64 ? 8 : 4);
    return 0;
}

int lcgp_sample_scratch_bytes(int dtype, int n0, int q_local, int S, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n0 < 1 || q_local < 1) return bad("n0, q_local must be >= 1");
    if (S < 1 || S > LCGP_SAMPLE_MAX) return bad("S must be in [1, 32768]");
    if (!bytes) return bad("bytes is NULL");
    *bytes = 2 * (size_t)q_local * round_up(S, 2 * TS) * cov_pad(n0) * (dtype == LCGP_F64 ? 8 : 4);
    return 0;
}

int lcgp_predict_cov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                     const double* theta, const void* workspace, int n0, const void* x0, int same, void* scratch,
                     void* cov_workspace, double jitter) {
    return cov_checked(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n0, x0, same, scratch,
                       cov_workspace, jitter);
}

int lcgp_sample_latent(void* stream, int dtype, int n0, int d, int p, int q_local, int S, void* cov_workspace, const void* eps,
                       const double* ghat, int ldg, void* scratch, double* out) {
    Ws cw;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n0, d, p, q_local, cov_workspace, cw, st);
    if (rc) return rc;
    if (S < 1 || S > LCGP_SAMPLE_MAX) return bad("S must be in [1, 32768]");
    if (ldg != 0 && ldg < n0) return bad("ldg must be 0 (= n0) or >= n0");
    if (!cov_workspace || !eps || !ghat || !scratch || !out) return bad("NULL pointer");
    const int ld = ldg ? ldg : n0;
    return by_dtype(dtype, [&](auto t) { return do_sample<decltype(t)>(st, cw, S, eps, ghat, ld, scratch, out); });
}

int lcgp_condition_scratch_bytes(int dtype, int n, int q_local, int m, int n0, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || q_local < 1) return bad("n, q_local must be >= 1");
    if (m < 1) return bad("m < 1");
    if (n0 < 0) return bad("n0 < 0");
    if (!bytes) return bad("bytes is NULL");
    const size_t a = cond_prepare_scratch(dtype, n, q_local, m);
    const size_t b = n0 ? cond_predict_scratch(dtype, n, q_local, m, n0) : 0;
    *bytes = a > b ? a : b;
    return 0;
}

int lcgp_condition_state_bytes(int dtype, int n, int d, int q_local, int m, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || q_local < 1) return bad("n, q_local must be >= 1");
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (m < 1) return bad("m < 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_carve(dtype, n, q_local, m).total;
    return 0;
}

int lcgp_condition_prepare(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                           const double* theta, const void* workspace, int m, const void* xn, const double* t, const double* r,
                           void* scratch, size_t scratch_bytes, void* cond_workspace, void* state, int* info) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (m < 1) return bad("m < 1");
    if (!x || !theta || !workspace || !xn || !t || !scratch || !cond_workspace || !state || !info) return bad("NULL pointer");
    if (scratch_bytes < cond_prepare_scratch(dtype, n, q_local, m))
        return bad("scratch is smaller than lcgp_condition_scratch_bytes(dtype, n, q_local, m, 0)");
    const Ws cw = carve(dtype, m, d, p, q_local, cond_workspace);
    return by_dtype(dtype, [&](auto t_) {
        return do_condition_prepare<decltype(t_)>(st, w, x, sr, theta, m, xn, t, r, scratch, cw, state, info);
    });
}

int lcgp_condition_predict(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                           const double* theta, const void* workspace, const void* state, int m, const void* xn, int n0,
                           const void* x0, void* scratch, size_t scratch_bytes, double* ghat, double* gvar, int out_stride) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    double* const o[6] = {ghat, gvar};
    return point_checked(PT_VALUE, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n0, x0, 0, scratch, o,
                         nullptr, out_stride);
}

int lcgp_condition_predict_marginal_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n0, size_t* bytes) {
    if (m < 0) return bad("m < 0");
    if (m == 0) return lcgp_predict_marginal_scratch_bytes(dtype, n, d, q_local, n0, bytes);
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || n0 < 1 || q_local < 1) return bad("n, n0, q_local must be >= 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_predict_scratch(dtype, n, q_local, m, n0)
             + (size_t)q_local * d * (round_up(n, 2 * TS) + 1 + cov_pad(m)) * sizeof(double);
    return 0;
}

int lcgp_condition_predict_marginal(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                    const void* sr, const double* theta, const void* workspace, const void* state, int m,
                                    const void* xn, int n0, const void* x0, const unsigned char* mask, const double* box,
                                    void* scratch, size_t scratch_bytes, double* ghat, double* gvar, int out_stride, int ref_row,
                                    void* ref_out, const void* ref_in, const void* ref_x, const unsigned char* ref_mask,
                                    double* gcov) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    MargRef ref;
    ref.row = ref_row; ref.out = ref_out; ref.in = ref_in; ref.x = ref_x; ref.mask = ref_mask; ref.gcov = gcov;
    return marginal_checked(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n0, x0, mask, box, scratch, ghat,
                            gvar, out_stride, ref);
}

int lcgp_condition_grad_state_bytes(int dtype, int n, int q_local, int m, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || q_local < 1) return bad("n, q_local must be >= 1");
    if (m < 1) return bad("m < 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_grad_carve(n, q_local, m).total;
    return 0;
}

int lcgp_condition_grad_prepare(void* stream, int dtype, int n, int d, int p, int q_local, const double* theta,
                                const void* workspace, const void* state, int m, void* grad_state) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (m < 1) return bad("m < 1");
    if (!theta || !workspace || !state || !grad_state) return bad("NULL pointer");
    return by_dtype(dtype, [&](auto t) { return do_condition_grad_prepare<decltype(t)>(st, w, theta, state, m, grad_state); });
}

int lcgp_condition_grad_fetch(void* stream, int n, int q_local, int m, const void* grad_state, double* w, double* z) {
    if (n < 1 || q_local < 1 || q_local > 65535) return bad("n must be >= 1, q_local in [1, 65535]");
    if (m < 1) return bad("m < 1");
    if (!grad_state || !w || !z) return bad("NULL pointer");
    const CondGradLay G = cond_grad_carve(n, q_local, m);
    const int big = n > m ? n : m;
    hipLaunchKernelGGL(cond_grad_fetch_kernel, dim3((big + 255) / 256, q_local), dim3(256), 0, (hipStream_t)stream,
                       (const double*)((const char*)grad_state + G.off_w), (int)cov_pad(m), m,
                       (const double*)((const char*)grad_state + G.off_z), round_up(n, 2 * TS), n, w, z);
    CHECK_LAUNCH("cond_grad_fetch_kernel");
    return 0;
}

int lcgp_condition_predict_grad_scratch_bytes(int dtype, int n, int q_local, int m, int n0, size_t* bytes) {
    if (dtype != LCGP_F64 && dtype != LCGP_F32) return bad("dtype must be 0 (f64) or 1 (f32)");
    if (n < 1 || q_local < 1) return bad("n, q_local must be >= 1");
    if (m < 1) return bad("m < 1");
    if (n0 < 1) return bad("n0 < 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_predict_scratch(dtype, n, q_local, m, n0);
    return 0;
}

int lcgp_condition_predict_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                const void* sr, const double* theta, const void* workspace, const void* state, int m,
                                const void* xn, const void* grad_state, int n0, const void* x0, void* scratch, size_t scratch_bytes,
                                double* ghat, double* gvar, double* dghat, double* dgvar, int out_stride) {
    const ViewArg v{state, m, xn, grad_state, scratch_bytes};
    double* const o[6] = {ghat, gvar, dghat, dgvar};
    return point_checked(PT_GRAD, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n0, x0, 0, scratch, o,
                         nullptr, out_stride);
}

int lcgp_condition_predict_hess_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n0, size_t* bytes) {
    return rows_bytes(true, dtype, n, d, q_local, &m, n0, bytes);
}

int lcgp_condition_predict_hess(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                const void* sr, const double* theta, const void* workspace, const void* state, int m,
                                const void* xn, const void* grad_state, int n0, const void* x0, void* scratch, size_t scratch_bytes,
                                double* ghat, double* gvar, double* dghat, double* dgvar, double* d2ghat, double* d2gvar,
                                int out_stride) {
    const ViewArg v{state, m, xn, grad_state, scratch_bytes};
    double* const o[6] = {ghat, gvar, dghat, dgvar, d2ghat, d2gvar};
    return point_checked(PT_HESS, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n0, x0, 0, scratch, o,
                         nullptr, out_stride);
}

int lcgp_condition_predict_gradcov_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n0, size_t* bytes) {
    return rows_bytes(false, dtype, n, d, q_local, &m, n0, bytes);
}

int lcgp_condition_predict_gradcov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                   const void* sr, const double* theta, const void* workspace, const void* state, int m,
                                   const void* xn, const void* grad_state, int n0, const void* x0, void* scratch,
                                   size_t scratch_bytes, double* dghat, double* gamma, const double* w, double* M, int out_stride) {
    const ViewArg v{state, m, xn, grad_state, scratch_bytes};
    double* const o[6] = {dghat, gamma, M};
    return point_checked(PT_GRADCOV, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n0, x0, 0, scratch, o,
                         w, out_stride);
}

int lcgp_loo(void* stream, int dtype, int n, int d, int p, int q_local, const void* sr, const double* theta,
             const void* workspace, double* ghat, double* gvar, int out_stride) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (!theta || !workspace || !ghat || !gvar) return bad("NULL pointer");
    if (out_stride != 0 && out_stride < n) return bad("out_stride must be 0 (= n) or >= n");
    const int ldo = out_stride ? out_stride : n;
    return by_dtype(dtype, [&](auto t) { return do_loo<decltype(t)>(st, w, sr, theta, ghat, gvar, ldo); });
}

int lcgp_cv_workspace_bytes(int dtype, int n, int d, int p, int q_local, int F, const int* folds_host, size_t* bytes) {
    int rc = check_common(dtype, n, d, p, q_local);
    if (rc) return rc;
    int mmax = 0;
    if ((rc = check_folds(n, q_local, F, folds_host, &mmax))) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = carve(dtype, mmax, d, p, q_local * F, nullptr).total;
    return 0;
}

int lcgp_cv_gather(void* stream, int dtype, int n, int d, int p, int q_local, const void* workspace, int F,
                   const int* folds_host, const int* folds, void* cv_workspace) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    int mmax = 0;
    if ((rc = check_folds(n, q_local, F, folds_host, &mmax))) return rc;
    if (!workspace || !folds || !cv_workspace) return bad("NULL pointer");
    const Ws cw = carve(dtype, mmax, d, p, q_local * F, cv_workspace);
    return by_dtype(dtype, [&](auto t) { return do_cv_gather<decltype(t)>(st, w, folds, F, cw); });
}

int lcgp_cv_apply(void* stream, int dtype, int n, int d, int p, int q_local, const void* sr, const double* theta,
                  const void* workspace, int F, const int* folds_host, const int* folds, const void* cv_workspace,
                  double* ghat, double* gvar, int out_stride) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, 0, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    int mmax = 0;
    if ((rc = check_folds(n, q_local, F, folds_host, &mmax))) return rc;
    if (!theta || !workspace || !folds || !cv_workspace || !ghat || !gvar) return bad("NULL pointer");
    if (out_stride != 0 && out_stride < n) return bad("out_stride must be 0 (= n) or >= n");
    const Ws cw = carve(dtype, mmax, d, p, q_local * F, (void*)cv_workspace);
    const int ldo = out_stride ? out_stride : n;
    return by_dtype(dtype, [&](auto t) { return do_cv_apply<decltype(t)>(st, w, sr, theta, folds, F, cw, ghat, gvar, ldo); });
}

// ---- variance reduction, its gradient (grad: the entry of lcgp_variance_reduction_grad, which takes no match) and their twins
// on a conditioned view (lcgp_hip.h: lcgp_condition_vr_*): the base model's code on widened rows (VrView) ----
static size_t vr_need(bool grad, int dtype, int n, int d, int q_local, int mpad, int n_ref, int n_cand) {
    return vr_carve(dtype, n, q_local, n_ref, n_cand, mpad).total +
           (grad ? vrg_carve(dtype, n, d, q_local, n_ref, n_cand, mpad).total : 0);
}

// m: the view's new inputs, NULL on the fitted model; the candidates of one gradient call are rows of a launch grid
static int vr_bytes(bool grad, int dtype, int n, int d, int q_local, const int* m, int n_ref, int n_cand, size_t* bytes) {
    int rc = check_common(dtype, n, d, 1, q_local);
    if (rc) return rc;
    if (m && (rc = check_view(*m))) return rc;
    if ((rc = check_vr(n_ref, n_cand))) return rc;
    if (grad && n_cand > 65535 - 2 * TS) return bad("n_cand must be <= 65407 per call (pass the candidates in chunks)");
    if (!bytes) return bad("bytes is NULL");
    *bytes = vr_need(grad, dtype, n, d, q_local, m ? cov_pad(*m) : 0, n_ref, n_cand);
    return 0;
}

static int vr_prepare_checked(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                              const double* theta, const void* workspace, const ViewArg* v, int n_ref, const void* x_ref,
                              void* scratch) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (v && (rc = check_view(v->m))) return rc;
    if ((rc = check_vr(n_ref, 1))) return rc;
    if (!x || !theta || !workspace || (v && (!v->state || !v->xn)) || !x_ref || !scratch) return bad("NULL pointer");
    if (v && v->scratch_bytes < vr_need(false, dtype, n, d, q_local, cov_pad(v->m), n_ref, 1))
        return bad("scratch is smaller than lcgp_condition_vr_scratch_bytes(dtype, n, q_local, m, n_ref, 1)");
    VrView cv;
    if (v) cv = view_of(dtype, n, q_local, *v);
    return by_dtype(dtype, [&](auto t) {
        return do_vr_prepare<decltype(t)>(st, w, x, sr, theta, n_ref, x_ref, (char*)scratch, v ? &cv : nullptr);
    });
}

static int vr_checked(bool grad, void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                      const void* sr, const double* theta, const void* workspace, const ViewArg* v, int n_ref, const void* x_ref,
                      const double* w_ref, int n_cand, const void* x_cand, const int* match_host, const int* match, int cand_row0,
                      int r, void* scratch, double* out, int out_stride, double* dout) {
    Ws w;
    hipStream_t st;
    int rc = open_entry(stream, dtype, kernel_id, n, d, p, q_local, workspace, w, st);
    if (rc) return rc;
    if (v && (rc = check_view(v->m))) return rc;
    if ((rc = check_vr(n_ref, n_cand))) return rc;
    if (grad && n_cand > 65535 - 2 * TS) return bad("n_cand must be <= 65407 per call (pass the candidates in chunks)");
    if (r < 1) return bad("r must be >= 1");
    if (cand_row0 < -1) return bad("cand_row0 must be -1 or a row of the reference set");
    if (cand_row0 >= 0) {
        if ((long long)cand_row0 + n_cand > n_ref) return bad("cand_row0 + n_cand must be <= n_ref");
        if (x_cand || match_host || match)
            return bad(grad ? "cand_row0 >= 0: x_cand must be NULL" : "cand_row0 >= 0: x_cand and match must be NULL");
    } else if (!x_cand) {
        return bad("NULL pointer");
    }
    if ((rc = check_match(n, n_cand, match_host, match))) return rc;
    if (!x || !theta || !workspace || (v && (!v->state || !v->xn)) || !x_ref || !w_ref || !scratch || !out || (grad && !dout))
        return bad("NULL pointer");
    if (out_stride != 0 && out_stride < n_cand) return bad("out_stride must be 0 (= n_cand) or >= n_cand");
    if (v && v->scratch_bytes < vr_need(grad, dtype, n, d, q_local, cov_pad(v->m), n_ref, n_cand))
        return bad(grad ? "scratch is smaller than lcgp_condition_vr_grad_scratch_bytes(dtype, n, d, q_local, m, n_ref, n_cand)"
                        : "scratch is smaller than lcgp_condition_vr_scratch_bytes(dtype, n, q_local, m, n_ref, n_cand)");
    const int ldo = out_stride ? out_stride : n_cand;
    VrView cv;
    if (v) cv = view_of(dtype, n, q_local, *v);
    const VrView* pcv = v ? &cv : nullptr;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return grad ? do_vr_grad<T>(st, w, x, sr, theta, n_ref, x_ref, w_ref, n_cand, x_cand, cand_row0, r, (char*)scratch, out, ldo,
                                    dout, pcv)
                    : do_vr<T>(st, w, x, sr, theta, n_ref, x_ref, w_ref, n_cand, x_cand, match, cand_row0, r, (char*)scratch, out,
                               ldo, pcv);
    });
}

int lcgp_variance_reduction_scratch_bytes(int dtype, int n, int q_local, int n_ref, int n_cand, size_t* bytes) {
    return vr_bytes(false, dtype, n, 1, q_local, nullptr, n_ref, n_cand, bytes);
}

int lcgp_variance_reduction_prepare(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                    const void* sr, const double* theta, const void* workspace, int n_ref, const void* x_ref,
                                    void* scratch) {
    return vr_prepare_checked(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n_ref, x_ref, scratch);
}

int lcgp_variance_reduction(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                            const double* theta, const void* workspace, int n_ref, const void* x_ref, const double* w_ref,
                            int n_cand, const void* x_cand, const int* match_host, const int* match, int cand_row0, int r,
                            void* scratch, double* out, int out_stride) {
    return vr_checked(false, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n_ref, x_ref, w_ref, n_cand,
                      x_cand, match_host, match, cand_row0, r, scratch, out, out_stride, nullptr);
}

int lcgp_variance_reduction_grad_scratch_bytes(int dtype, int n, int d, int q_local, int n_ref, int n_cand, size_t* bytes) {
    return vr_bytes(true, dtype, n, d, q_local, nullptr, n_ref, n_cand, bytes);
}

int lcgp_variance_reduction_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                 const void* sr, const double* theta, const void* workspace, int n_ref, const void* x_ref,
                                 const double* w_ref, int n_cand, const void* x_cand, int cand_row0, int r, void* scratch,
                                 double* out, int out_stride, double* dout) {
    return vr_checked(true, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n_ref, x_ref, w_ref, n_cand,
                      x_cand, nullptr, nullptr, cand_row0, r, scratch, out, out_stride, dout);
}

// ---- greedy selection and its twins on a conditioned view (lcgp_hip.h: lcgp_select_* / lcgp_condition_select_*) ----
// What the five entries test first, on the fitted model (m == NULL) and on a view of *m new inputs; *L receives the layout.  A view
// entry is told the size of its scratch and tests it here, so its scratch pointer too; the model entries test theirs with their
// other pointers, behind their own arguments.
static int open_sel(int dtype, int n, int d, int p, int q_local, int kernel_id, const int* m, int n_ref, int n_cand, int size,
                    const void* scratch, size_t scratch_bytes, SelLay* L) {
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    if (m && (rc = check_view(*m))) return rc;
    if ((rc = check_sel(n_ref, n_cand, size))) return rc;
    if (m && !scratch) return bad("NULL pointer");
    *L = sel_carve(dtype, n, d, q_local, n_ref, n_cand, size, m ? cov_pad(*m) : 0);
    if (m && scratch_bytes < L->total)
        return bad("scratch is smaller than lcgp_condition_select_scratch_bytes(dtype, n, d, q_local, m, n_ref, n_cand, size)");
    return 0;
}

static int sel_bytes(int dtype, int n, int d, int q_local, const int* m, int n_ref, int n_cand, int size, size_t* bytes) {
    int rc = check_common(dtype, n, d, 1, q_local);
    if (rc) return rc;
    if (m && (rc = check_view(*m))) return rc;
    if ((rc = check_sel(n_ref, n_cand, size))) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = sel_carve(dtype, n, d, q_local, n_ref, n_cand, size, m ? cov_pad(*m) : 0).total;
    return 0;
}

static int sel_begin(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                     const double* theta, const void* workspace, const ViewArg* v, int n_ref, const void* x_ref, const double* w_ref,
                     int n_cand, const void* x_cand, const int* match_host, const int* match, int r, int size, int pass_rows,
                     void* scratch) {
    SelLay L;
    int rc = open_sel(dtype, n, d, p, q_local, kernel_id, v ? &v->m : nullptr, n_ref, n_cand, size, scratch, v ? v->scratch_bytes : 0, &L);
    if (rc) return rc;
    if (r < 1) return bad("r must be >= 1");
    if (pass_rows < 1 || pass_rows > VR_XBLK) return bad("pass_rows must be in [1, 2048]");
    if ((rc = check_match(n, n_cand, match_host, match))) return rc;
    if (!x || !theta || !workspace || (v && (!v->state || !v->xn)) || !x_ref || !w_ref || !x_cand || !scratch)
        return bad("NULL pointer");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    w.kern = kernel_id;
    VrView cv;
    if (v) cv = view_of(dtype, n, q_local, *v);
    return by_dtype(dtype, [&](auto t) {
        return do_sel_begin<decltype(t)>((hipStream_t)stream, w, x, sr, theta, n_ref, x_ref, w_ref, n_cand, x_cand, match, r, size,
                                         pass_rows, (char*)scratch, v ? &cv : nullptr);
    });
}

static int sel_score(void* stream, int dtype, int n, int d, int q_local, const int* m, int n_ref, int n_cand, int size, int step,
                     const double* omega, void* scratch, size_t scratch_bytes, double* out) {
    SelLay L;
    int rc = open_sel(dtype, n, d, 1, q_local, 0, m, n_ref, n_cand, size, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (step < 0 || step >= size) return bad("step must be in [0, size)");
    if (!omega || !scratch) return bad("NULL pointer");
    char* sc = (char*)scratch;
    hipLaunchKernelGGL(sel_score_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)(sc + L.off_R), q_local, n_cand,
                       omega, (const int*)(sc + L.off_mask), out, (int*)(sc + L.off_picks) + step);
    CHECK_LAUNCH("sel_score_kernel");
    return 0;
}

static int sel_picks(int dtype, int n, int d, int q_local, const int* m, int n_ref, int n_cand, int size, void* scratch,
                     size_t scratch_bytes, int** picks) {
    SelLay L;
    int rc = open_sel(dtype, n, d, 1, q_local, 0, m, n_ref, n_cand, size, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (!scratch || !picks) return bad("NULL pointer");
    *picks = (int*)((char*)scratch + L.off_picks);
    return 0;
}

static int sel_condition(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* theta, const int* m,
                         int n_ref, int n_cand, int size, int r, int step, const int* pick, void* scratch, size_t scratch_bytes) {
    SelLay L;
    int rc = open_sel(dtype, n, d, p, q_local, kernel_id, m, n_ref, n_cand, size, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (r < 1) return bad("r must be >= 1");
    if (step < 0 || step >= size) return bad("step must be in [0, size)");
    if (!theta || !pick || !scratch) return bad("NULL pointer");
    Ws w;
    memset(&w, 0, sizeof(w));
    w.n = n; w.npad = round_up(n, 2 * TS); w.d = d; w.p = p; w.q = q_local; w.kern = kernel_id;
    w.esz = dtype == LCGP_F64 ? 8 : 4;
    return by_dtype(dtype, [&](auto t) {
        return do_sel_condition<decltype(t)>((hipStream_t)stream, w, theta, n_ref, n_cand, size, r, step, pick, (char*)scratch,
                                             m ? cov_pad(*m) : 0);
    });
}

static int sel_state(void* stream, int dtype, int n, int d, int q_local, const int* m, int n_ref, int n_cand, int size, int which,
                     const void* scratch, size_t scratch_bytes, double* out) {
    SelLay L;
    int rc = open_sel(dtype, n, d, 1, q_local, 0, m, n_ref, n_cand, size, scratch, scratch_bytes, &L);
    if (rc) return rc;
    if (which != 0 && which != 1) return bad("which must be 0 (R) or 1 (h)");
    if (!scratch || !out) return bad("NULL pointer");
    hipError_t e = hipMemcpyAsync(out, (const char*)scratch + (which ? L.off_h : L.off_R), (size_t)q_local * n_cand * sizeof(double),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? 0 : fail("hipMemcpyAsync", e);
}

int lcgp_select_scratch_bytes(int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, size_t* bytes) {
    return sel_bytes(dtype, n, d, q_local, nullptr, n_ref, n_cand, size, bytes);
}

int lcgp_select_begin(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                      const double* theta, const void* workspace, int n_ref, const void* x_ref, const double* w_ref, int n_cand,
                      const void* x_cand, const int* match_host, const int* match, int r, int size, int pass_rows, void* scratch) {
    return sel_begin(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, nullptr, n_ref, x_ref, w_ref, n_cand, x_cand,
                     match_host, match, r, size, pass_rows, scratch);
}

int lcgp_select_score(void* stream, int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, int step,
                      const double* omega, void* scratch, double* out) {
    return sel_score(stream, dtype, n, d, q_local, nullptr, n_ref, n_cand, size, step, omega, scratch, 0, out);
}

int lcgp_select_picks(int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, void* scratch, int** picks) {
    return sel_picks(dtype, n, d, q_local, nullptr, n_ref, n_cand, size, scratch, 0, picks);
}

int lcgp_select_condition(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* theta,
                          int n_ref, int n_cand, int size, int r, int step, const int* pick, void* scratch) {
    return sel_condition(stream, dtype, kernel_id, n, d, p, q_local, theta, nullptr, n_ref, n_cand, size, r, step, pick, scratch, 0);
}

int lcgp_select_state(void* stream, int dtype, int n, int d, int q_local, int n_ref, int n_cand, int size, int which,
                      const void* scratch, double* out) {
    return sel_state(stream, dtype, n, d, q_local, nullptr, n_ref, n_cand, size, which, scratch, 0, out);
}

int lcgp_condition_vr_scratch_bytes(int dtype, int n, int q_local, int m, int n_ref, int n_cand, size_t* bytes) {
    return vr_bytes(false, dtype, n, 1, q_local, &m, n_ref, n_cand, bytes);
}

int lcgp_condition_vr_prepare(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                              const double* theta, const void* workspace, const void* state, int m, const void* xn, int n_ref,
                              const void* x_ref, void* scratch, size_t scratch_bytes) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    return vr_prepare_checked(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n_ref, x_ref, scratch);
}

int lcgp_condition_vr(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                      const double* theta, const void* workspace, const void* state, int m, const void* xn, int n_ref,
                      const void* x_ref, const double* w_ref, int n_cand, const void* x_cand, const int* match_host, const int* match,
                      int cand_row0, int r, void* scratch, size_t scratch_bytes, double* out, int out_stride) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    return vr_checked(false, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n_ref, x_ref, w_ref, n_cand,
                      x_cand, match_host, match, cand_row0, r, scratch, out, out_stride, nullptr);
}

int lcgp_condition_vr_grad_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, size_t* bytes) {
    return vr_bytes(true, dtype, n, d, q_local, &m, n_ref, n_cand, bytes);
}

int lcgp_condition_vr_grad(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                           const double* theta, const void* workspace, const void* state, int m, const void* xn, int n_ref,
                           const void* x_ref, const double* w_ref, int n_cand, const void* x_cand, int cand_row0, int r,
                           void* scratch, size_t scratch_bytes, double* out, int out_stride, double* dout) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    return vr_checked(true, stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n_ref, x_ref, w_ref, n_cand,
                      x_cand, nullptr, nullptr, cand_row0, r, scratch, out, out_stride, dout);
}

// ---- joint posterior covariance of a conditioned view (lcgp_hip.h) ----
int lcgp_condition_predict_cov_scratch_bytes(int dtype, int n, int q_local, int m, int n0, size_t* bytes) {
    int rc = check_common(dtype, n, 1, 1, q_local);
    if (rc) return rc;
    if ((rc = check_view(m))) return rc;
    if (n0 < 1) return bad("n0 < 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_cov_carve(dtype, n, q_local, m, n0).total;
    return 0;
}

int lcgp_condition_predict_cov(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                               const void* sr, const double* theta, const void* workspace, const void* state, int m, const void* xn,
                               int n0, const void* x0, void* scratch, size_t scratch_bytes, void* cov_workspace, double jitter) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    return cov_checked(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n0, x0, 0, scratch, cov_workspace,
                       jitter);
}

int lcgp_condition_select_scratch_bytes(int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size, size_t* bytes) {
    return sel_bytes(dtype, n, d, q_local, &m, n_ref, n_cand, size, bytes);
}

int lcgp_condition_select_begin(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x,
                                const void* sr, const double* theta, const void* workspace, const void* state, int m, const void* xn,
                                int n_ref, const void* x_ref, const double* w_ref, int n_cand, const void* x_cand,
                                const int* match_host, const int* match, int r, int size, int pass_rows, void* scratch,
                                size_t scratch_bytes) {
    const ViewArg v{state, m, xn, nullptr, scratch_bytes};
    return sel_begin(stream, dtype, kernel_id, n, d, p, q_local, x, sr, theta, workspace, &v, n_ref, x_ref, w_ref, n_cand, x_cand,
                     match_host, match, r, size, pass_rows, scratch);
}

int lcgp_condition_select_score(void* stream, int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size, int step,
                                const double* omega, void* scratch, size_t scratch_bytes, double* out) {
    return sel_score(stream, dtype, n, d, q_local, &m, n_ref, n_cand, size, step, omega, scratch, scratch_bytes, out);
}

int lcgp_condition_select_picks(int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size, void* scratch,
                                size_t scratch_bytes, int** picks) {
    return sel_picks(dtype, n, d, q_local, &m, n_ref, n_cand, size, scratch, scratch_bytes, picks);
}

int lcgp_condition_select_condition(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* theta,
                                    int m, int n_ref, int n_cand, int size, int r, int step, const int* pick, void* scratch,
                                    size_t scratch_bytes) {
    return sel_condition(stream, dtype, kernel_id, n, d, p, q_local, theta, &m, n_ref, n_cand, size, r, step, pick, scratch,
                         scratch_bytes);
}

int lcgp_condition_select_state(void* stream, int dtype, int n, int d, int q_local, int m, int n_ref, int n_cand, int size, int which,
                                const void* scratch, size_t scratch_bytes, double* out) {
    return sel_state(stream, dtype, n, d, q_local, &m, n_ref, n_cand, size, which, scratch, scratch_bytes, out);
}

int lcgp_calib_rows(void* stream, int q, int d, int n0, const double* ghat, const double* gvar, const double* dghat,
                    const double* dgvar, int in_stride, const double* M, const double* b, double c0, double lognorm,
                    const double* inv_range, double* ll, double* dll, double* sens) {
    if (q < 1 || q > LCGP_CALIB_MAX_Q) return bad("q must be in [1, LCGP_CALIB_MAX_Q = 64]");
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (n0 < 1) return bad("n0 < 1");
    if (!ghat || !gvar || !M || !b || !ll) return bad("NULL pointer");
    if ((dghat == nullptr) != (dgvar == nullptr)) return bad("dghat and dgvar must both be given or both be NULL");
    if (dll && !dghat) return bad("dll needs the Jacobians dghat and dgvar");
    if (in_stride != 0 && in_stride < n0) return bad("in_stride must be 0 (= n0) or >= n0");
    const size_t ld = in_stride ? in_stride : n0;
    hipStream_t st = (hipStream_t)stream;
    switch (q) {
#define LCGP_CALIB_CASE(Q) \
    case Q: return launch_calib_small<Q>(st, d, n0, ghat, gvar, dghat, dgvar, ld, M, b, c0, lognorm, inv_range, ll, dll, sens);
        LCGP_CALIB_CASE(1) LCGP_CALIB_CASE(2) LCGP_CALIB_CASE(3) LCGP_CALIB_CASE(4)
        LCGP_CALIB_CASE(5) LCGP_CALIB_CASE(6) LCGP_CALIB_CASE(7) LCGP_CALIB_CASE(8)
#undef LCGP_CALIB_CASE
        default: break;
    }
    hipLaunchKernelGGL(calib_rows_wave_kernel, dim3(n0), dim3(64), 2 * (size_t)q * q * sizeof(double), st, q, d, n0, ghat, gvar,
                       dghat, dgvar, ld, M, b, c0, lognorm, inv_range, ll, dll, sens);
    CHECK_LAUNCH("calib_rows_wave");
    return 0;
}

int lcgp_calib_hess_rows(void* stream, int q, int d, int n0, const double* ghat, const double* gvar, const double* dghat,
                         const double* dgvar, const double* d2ghat, const double* d2gvar, int in_stride, const double* M,
                         const double* b, double c0, double lognorm, const double* inv_range, double* ll, double* dll,
                         double* d2ll, double* sens, double* Bout) {
    if ((d2ghat == nullptr) != (d2gvar == nullptr)) return bad("d2ghat and d2gvar must both be given or both be NULL");
    if (d2ll && !d2ghat) return bad("d2ll needs the Hessians d2ghat and d2gvar");
    if (d2ll && !dghat) return bad("d2ll needs the Jacobians dghat and dgvar");
    // (every other check is lcgp_calib_rows', made there before its launch; the second launch adds no condition of its own)
    int rc = lcgp_calib_rows(stream, q, d, n0, ghat, gvar, dghat, dgvar, in_stride, M, b, c0, lognorm, inv_range, ll, dll, sens);
    if (rc || (!d2ll && !Bout)) return rc;
    const size_t ld = in_stride ? in_stride : n0;
    hipLaunchKernelGGL(calib_hess_wave_kernel, dim3(n0), dim3(64), 2 * (size_t)q * q * sizeof(double), (hipStream_t)stream, q, d, n0,
                       ghat, gvar, dghat, dgvar, ld, M, b, inv_range, d2ghat, d2gvar, d2ll, Bout);
    CHECK_LAUNCH("calib_hess_wave");
    return 0;
}

static int sobol_check(int n, int d, int q_all, int npairs) {
    if (n < 1) return bad("n < 1");
    if (d < 1 || d > DWIDE) return bad("d must be in [1, 126]");
    if (q_all < 1 || q_all > 65535) return bad("q_all must be in [1, 65535]");
    if (npairs < 1) return bad("npairs < 1");
    if ((n + TS - 1) / TS > 65535) return bad("n must be at most 64 * 65535");
    return 0;
}

int lcgp_sobol_scratch_bytes(int n, int d, int q_all, int npairs, size_t* bytes) {
    int rc = sobol_check(n, d, q_all, npairs);
    if (rc) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = ((size_t)q_all * d * n + q_all + sobol_part_doubles(n, d, npairs)) * sizeof(double);
    return 0;
}

int lcgp_sobol_pairs(void* stream, int kernel_id, int n, int d, int q_all, const double* x, const double* w, const double* ell,
                     const double* box, const int* pairs, int npairs, void* scratch, double* out) {
    if (kernel_id != LCGP_KERNEL_MATERN32 && kernel_id != LCGP_KERNEL_SE && kernel_id != LCGP_KERNEL_MATERN52)
        return bad("kernel_id must be 0 (Matern-3/2), 1 (squared exponential) or 2 (Matern-5/2)");
    int rc = sobol_check(n, d, q_all, npairs);
    if (rc) return rc;
    if (!x || !w || !ell || !box || !pairs || !scratch || !out) return bad("NULL pointer");
    for (int i = 0; i < 2 * npairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= q_all) return bad("pairs must hold component indices in [0, q_all)");
    return do_sobol_pairs<SOBOL_VEC>((hipStream_t)stream, kernel_id, n, d, q_all, x, w, ell, box, pairs, npairs, scratch, out,
                                 SobolQ{nullptr, 0, 0});
}

// ks: local component indices, scanned here; pairs (the entries on the fitted model) receives the pairs (k, k)
static int check_ks(const int* ks, int nks, int q_local, std::vector<int>* pairs = nullptr) {
    for (int i = 0; i < nks; ++i) {
        if (ks[i] < 0 || ks[i] >= q_local) return bad("ks must hold local component indices in [0, q_local)");
        if (pairs) pairs->insert(pairs->end(), 2, ks[i]);
    }
    return 0;
}

int lcgp_sobol_matrix_scratch_bytes(int n, int d, int q_local, int nks, size_t* bytes) {
    int rc = sobol_check(n, d, q_local, 1);
    if (rc) return rc;
    if (nks < 1) return bad("nks < 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = ((size_t)q_local * d * n + q_local + sobol_part_doubles(n, d, nks, 1)) * sizeof(double);
    return 0;
}

int lcgp_sobol_matrix_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* x,
                            const double* v, const double* ell, const double* box, const void* workspace, const int* ks,
                            int nks, void* scratch, double* out) {
    if (dtype != LCGP_F64) return bad("lcgp_sobol_matrix_pairs reads a float64 workspace");
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    if ((rc = sobol_check(n, d, q_local, 1))) return rc;
    if (nks < 1) return bad("nks < 1");
    if (!x || !v || !ell || !box || !workspace || !ks || !scratch || !out) return bad("NULL pointer");
    std::vector<int> pairs;
    if ((rc = check_ks(ks, nks, q_local, &pairs))) return rc;
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    const SobolQ qm{(const double*)(w.base + w.off_V), w.mat, w.npad};
    return do_sobol_pairs<SOBOL_MAT>((hipStream_t)stream, kernel_id, n, d, q_local, x, v, ell, box, pairs.data(), nks, scratch, out, qm);
}

static int cond_sobol_check(int n, int d, int q_local, int m, int nks) {
    if (m < 1) return bad("m < 1");
    if (n > INT_MAX - m) return bad("n + m overflows");
    int rc = sobol_check(n + m, d, q_local, 1);
    if (rc) return rc;
    if (nks < 1) return bad("nks < 1");
    return 0;
}

int lcgp_condition_sobol_scratch_bytes(int n, int d, int q_local, int m, int nks, size_t* bytes) {
    if (n < 1) return bad("n < 1");
    int rc = cond_sobol_check(n, d, q_local, m, nks);
    if (rc) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_sobol_carve(n, d, q_local, m).total;
    return 0;
}

int lcgp_condition_sobol_matrix_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* theta,
                                      const void* workspace, const void* state, int m, const double* xa, const double* v,
                                      const double* ell, const double* box, const int* ks, int nks, void* scratch,
                                      size_t scratch_bytes, double* out) {
    if (dtype != LCGP_F64) return bad("lcgp_condition_sobol_matrix_pairs reads a float64 workspace and a float64 state");
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    if ((rc = cond_sobol_check(n, d, q_local, m, nks))) return rc;
    if (!theta || !workspace || !state || !xa || !v || !ell || !box || !ks || !scratch || !out) return bad("NULL pointer");
    if ((rc = check_ks(ks, nks, q_local))) return rc;
    if (scratch_bytes < cond_sobol_carve(n, d, q_local, m).total) return bad("scratch too small (lcgp_condition_sobol_scratch_bytes)");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    w.kern = kernel_id;
    return do_condition_sobol((hipStream_t)stream, w, theta, state, m, xa, v, ell, box, ks, nks, scratch, out);
}

// ---- closed variances of a caller's input subsets ----
int lcgp_sobol_subset_chunk(int d) {
    if (d < 1 || d > SOBOL_SUBSET_DMAX) return bad("the subset pass takes d in [1, 16]");
    return sobol_subset_chunk(d);
}

static int sobol_subset_check(int n, int d, int q_all, int npairs, int nsub) {
    if (d > SOBOL_SUBSET_DMAX) return bad("the subset pass takes d in [1, 16] (a mask addresses 16 inputs; no d > 16 variant)");
    int rc = sobol_check(n, d, q_all, npairs);
    if (rc) return rc;
    if (nsub < 1) return bad("nsub < 1");
    return 0;
}

static int sobol_masks_check(const uint64_t* masks, int nsub, int d) {
    for (int s = 0; s < nsub; ++s)
        if (masks[s] >> d) return bad("a mask has a bit at or above d");
    return 0;
}

int lcgp_sobol_subset_scratch_bytes(int n, int d, int q_all, int npairs, int nsub, size_t* bytes) {
    int rc = sobol_subset_check(n, d, q_all, npairs, nsub);
    if (rc) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = ((size_t)q_all * d * n + q_all + sobol_subset_part_doubles(n, d, npairs)) * sizeof(double);
    return 0;
}

int lcgp_sobol_subset_pairs(void* stream, int kernel_id, int n, int d, int q_all, const double* x, const double* w,
                            const double* ell, const double* box, const int* pairs, int npairs, const uint64_t* masks, int nsub,
                            void* scratch, double* out) {
    if (kernel_id != LCGP_KERNEL_MATERN32 && kernel_id != LCGP_KERNEL_SE && kernel_id != LCGP_KERNEL_MATERN52)
        return bad("kernel_id must be 0 (Matern-3/2), 1 (squared exponential) or 2 (Matern-5/2)");
    int rc = sobol_subset_check(n, d, q_all, npairs, nsub);
    if (rc) return rc;
    if (!x || !w || !ell || !box || !pairs || !masks || !scratch || !out) return bad("NULL pointer");
    for (int i = 0; i < 2 * npairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= q_all) return bad("pairs must hold component indices in [0, q_all)");
    if ((rc = sobol_masks_check(masks, nsub, d))) return rc;
    return do_sobol_subset_pairs<SOBOL_VEC>((hipStream_t)stream, kernel_id, n, d, q_all, x, w, ell, box, pairs, npairs, masks, nsub,
                                            scratch, out, SobolQ{nullptr, 0, 0});
}

int lcgp_sobol_matrix_subset_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const double* x,
                                   const double* v, const double* ell, const double* box, const void* workspace, const int* ks,
                                   int nks, const uint64_t* masks, int nsub, void* scratch, double* out) {
    if (dtype != LCGP_F64) return bad("lcgp_sobol_matrix_subset_pairs reads a float64 workspace");
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    if ((rc = sobol_subset_check(n, d, q_local, 1, nsub))) return rc;
    if (nks < 1) return bad("nks < 1");
    if (!x || !v || !ell || !box || !workspace || !ks || !masks || !scratch || !out) return bad("NULL pointer");
    std::vector<int> pairs;
    if ((rc = check_ks(ks, nks, q_local, &pairs))) return rc;
    if ((rc = sobol_masks_check(masks, nsub, d))) return rc;
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    const SobolQ qm{(const double*)(w.base + w.off_V), w.mat, w.npad};
    return do_sobol_subset_pairs<SOBOL_MAT>((hipStream_t)stream, kernel_id, n, d, q_local, x, v, ell, box, pairs.data(), nks, masks,
                                            nsub, scratch, out, qm);
}

int lcgp_condition_sobol_subset_scratch_bytes(int n, int d, int q_local, int m, int nks, int nsub, size_t* bytes) {
    if (n < 1) return bad("n < 1");
    if (d > SOBOL_SUBSET_DMAX) return bad("the subset pass takes d in [1, 16] (a mask addresses 16 inputs; no d > 16 variant)");
    int rc = cond_sobol_check(n, d, q_local, m, nks);
    if (rc) return rc;
    if (nsub < 1) return bad("nsub < 1");
    if (!bytes) return bad("bytes is NULL");
    *bytes = cond_sobol_carve(n, d, q_local, m, true).total;
    return 0;
}

int lcgp_condition_sobol_matrix_subset_pairs(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local,
                                             const double* theta, const void* workspace, const void* state, int m, const double* xa,
                                             const double* v, const double* ell, const double* box, const int* ks, int nks,
                                             const uint64_t* masks, int nsub, void* scratch, size_t scratch_bytes, double* out) {
    if (dtype != LCGP_F64) return bad("lcgp_condition_sobol_matrix_subset_pairs reads a float64 workspace and a float64 state");
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    if (d > SOBOL_SUBSET_DMAX) return bad("the subset pass takes d in [1, 16] (a mask addresses 16 inputs; no d > 16 variant)");
    if ((rc = cond_sobol_check(n, d, q_local, m, nks))) return rc;
    if (nsub < 1) return bad("nsub < 1");
    if (!theta || !workspace || !state || !xa || !v || !ell || !box || !ks || !masks || !scratch || !out) return bad("NULL pointer");
    if ((rc = check_ks(ks, nks, q_local))) return rc;
    if ((rc = sobol_masks_check(masks, nsub, d))) return rc;
    if (scratch_bytes < cond_sobol_carve(n, d, q_local, m, true).total)
        return bad("scratch too small (lcgp_condition_sobol_subset_scratch_bytes)");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    w.kern = kernel_id;
    return do_condition_sobol((hipStream_t)stream, w, theta, state, m, xa, v, ell, box, ks, nks, scratch, out, masks, nsub);
}

static int check_box_alc(int dtype, int n_cand) {
    if (dtype != LCGP_F64) return bad("lcgp_box_alc reads a float64 workspace (its three terms cancel): evaluate on a float64 workspace");
    if (n_cand < 1) return bad("n_cand must be >= 1");
    if (n_cand > 65535) return bad("n_cand must be <= 65535: pass the candidates in chunks");
    return 0;
}

int lcgp_box_alc_scratch_bytes(int dtype, int n, int d, int q_group, int n_cand, size_t* bytes) {
    int rc = check_common(dtype, n, d, 1, q_group);
    if (rc) return rc;
    if ((rc = check_box_alc(dtype, n_cand))) return rc;
    if (!bytes) return bad("bytes is NULL");
    *bytes = box_carve(n, q_group, n_cand).total;
    return 0;
}

int lcgp_box_alc(void* stream, int dtype, int kernel_id, int n, int d, int p, int q_local, const void* x, const void* sr,
                 const double* theta, const void* workspace, int k0, int q_group, const double* box, int n_cand,
                 const void* x_cand, const int* match, int replicates, int form_m, void* scratch, double* out, int out_stride) {
    int rc = check_common(dtype, n, d, p, q_local, kernel_id);
    if (rc) return rc;
    if ((rc = check_box_alc(dtype, n_cand))) return rc;
    if (k0 < 0 || q_group < 1 || k0 + q_group > q_local) return bad("k0 / q_group must select components inside [0, q_local)");
    if (!x || !theta || !workspace || !box || !x_cand || !scratch || !out) return bad("NULL pointer");
    if (replicates < 1) return bad("replicates must be >= 1");
    if (out_stride != 0 && out_stride < n_cand) return bad("out_stride must be 0 (= n_cand) or >= n_cand");
    Ws w = carve(dtype, n, d, p, q_local, (void*)workspace);
    w.kern = kernel_id;
    return do_box_alc((hipStream_t)stream, w, x, sr, theta, k0, q_group, box, n_cand, x_cand, match, replicates, form_m,
                      (char*)scratch, out, out_stride ? out_stride : n_cand);
}

}  // extern "C"
