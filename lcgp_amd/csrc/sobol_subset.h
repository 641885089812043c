// sobol_subset.h -- the subset product behind the closed variances of arbitrary input subsets (lcgp_sobol_subset_pairs;
// DESIGN.md 4.25).  Host and device: the kernel (lcgp_hip.hip, sobol_subset_kernel) and the CPU test that checks these few lines
// against the numpy restatement (tests/test_sobol_subset_host.py) compile the same text.
//
// Per element (i, i') and input l the kernel holds J[l] (the pair average of the two 1-D factors) and A[l] = a_l[i] a'_l[i'] (the
// product of their single averages).  For a subset u given as a bit mask (bit l set: input l is in u)
//     P_u = prod_l (bit_l ? J[l] : A[l]),      l ascending,
// a select per factor, never a division: factors may underflow to zero.  M_0 = P of the empty mask, the same loop, so the
// difference P_u - M_0 of the empty mask is exactly 0.0.  Nothing here may be contracted into a fused multiply-add: the product
// and the difference of one mask must round the same way wherever the mask stands in a launch and on host and device alike.
#ifndef LCGP_SOBOL_SUBSET_H
#define LCGP_SOBOL_SUBSET_H

#if defined(__HIPCC__)
#define LCGP_SUBSET_HD __host__ __device__ __forceinline__
#else
#define LCGP_SUBSET_HD inline
#endif

constexpr int SOBOL_SUBSET_DMAX = 16;         // no subset path beyond: a mask addresses the inputs 0 .. 15

// masks per launch for the instance with DD padded dimensions (DD = 8: d <= 8; DD = 16: d <= 16): the accumulators live in
// registers (2 VGPRs each), beside the 2 DD factors of the element
constexpr int sobol_subset_chunk(int dd) { return dd <= 8 ? 32 : 32; }

// prod_l (bit_l ? J[l] : A[l]); dimensions d .. DD - 1 hold J = A = 1 and no mask has a bit there
template <int DD>
LCGP_SUBSET_HD double sobol_subset_product(unsigned mask, const double (&J)[DD], const double (&A)[DD]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double p = 1.0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int l = 0; l < DD; ++l) p = p * (((mask >> l) & 1u) ? J[l] : A[l]);
    return p;
}

// P_u - M_0 with m0 = sobol_subset_product(0, J, A)
template <int DD>
LCGP_SUBSET_HD double sobol_subset_diff(unsigned mask, const double (&J)[DD], const double (&A)[DD], double m0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = sobol_subset_product<DD>(mask, J, A);
    return p - m0;
}

#endif  // LCGP_SOBOL_SUBSET_H
