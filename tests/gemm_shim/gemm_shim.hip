// gemm_shim.hip - test-only entry points over awesome_amd/csrc/gemm.h (tests/gemm_cases.py builds libgemm_shim.so from it; nothing of
// this is part of libinrfit.so or its ABI).  GemmShimArgs is the shim's OWN struct: it is copied field by field into GemmArgs here, so
// a change of GemmArgs breaks this compile instead of misaligning a ctypes mirror.
#include "../../awesome_amd/csrc/gemm.h"

#define SHIM_API extern "C" __attribute__((visibility("default")))

extern "C" {
struct GemmShimArgs {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    const float* skip;
    const float* ext;
    const float* mask;
    float* extsum;
    long long c_split_stride;
    int tA, tB;
    int M, N, K, lda, ldb, ldc;
    int k_per_split;
    int epi;
    int ext_ld, C_in, ext_copy;
    int mask_ld, mask_act;
    float omega;
    int buf, c_zero_to, padA, padB;
};
}

static GemmArgs shim_args(const GemmShimArgs* a) {
    GemmArgs g{};
    g.A = a->A; g.B = a->B; g.C = a->C;
    g.M = a->M; g.N = a->N; g.K = a->K; g.lda = a->lda; g.ldb = a->ldb; g.ldc = a->ldc;
    g.k_per_split = a->k_per_split;
    g.c_split_stride = a->c_split_stride;
    g.epi = a->epi;
    g.bias = a->bias; g.skip = a->skip; g.ext = a->ext;
    g.ext_ld = a->ext_ld; g.C_in = a->C_in; g.ext_copy = a->ext_copy;
    g.mask = a->mask; g.mask_ld = a->mask_ld; g.mask_act = a->mask_act;
    g.omega = a->omega;
    g.buf = a->buf; g.c_zero_to = a->c_zero_to;
    g.extsum = a->extsum;
    g.padA = a->padA; g.padB = a->padB;
    return g;
}

SHIM_API int gemm_shim_args_size(void) { return (int)sizeof(GemmShimArgs); }
// constants of gemm.h the tests size their buffers by: 0 GM_BK, 1 GM_BM, 2 GM_BN, 3 GEMM_SPLITK_MAX
SHIM_API int gemm_shim_const(int which) {
    const int v[4] = {GM_BK, GM_BM, GM_BN, GEMM_SPLITK_MAX};
    return which >= 0 && which < 4 ? v[which] : -1;
}
SHIM_API int gemm_shim_splitk_len(int K) { return gemm_splitk_len(K); }

// one launch on the default stream (asynchronous, like every launch of the library)
SHIM_API int gemm_shim_launch(const GemmShimArgs* a) { return gemm_launch(nullptr, a->tA != 0, a->tB != 0, shim_args(a)); }

// gemm_rm_splitk: C dense [M][N], part [GEMM_SPLITK_MAX][M][N]
SHIM_API int gemm_shim_splitk(int tA, int tB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, float* part) {
    return gemm_rm_splitk(nullptr, tA != 0, tB != 0, M, N, K, A, lda, B, ldb, C, part);
}

// which kernel gemm_launch would pick: returns MODE (0 general, 1 V4, 2 buffer descriptors); *vecA / *vecB the operands' widest aligned
// loads, *buf GemmArgs::buf after the 2 GiB fallback.  Host arithmetic only: the pointers are never dereferenced.
SHIM_API int gemm_shim_pick_mode(const GemmShimArgs* a, int* vecA, int* vecB, int* buf) {
    GemmArgs g = shim_args(a);
    const int mode = gemm_pick_mode(a->tA != 0, a->tB != 0, g);
    if (vecA) *vecA = g.vecA;
    if (vecB) *vecB = g.vecB;
    if (buf) *buf = g.buf;
    return mode;
}
