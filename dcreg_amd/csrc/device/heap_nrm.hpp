// The heap of the searches that need their neighbours' IDENTITIES in rank order: the normals (normals.hip k_nrm) and the descriptors
// (features.hip k_fpfh_spfh).  The ring walk itself is search.hpp's knn_search.
#pragma once
#include "search.hpp"

namespace dcreg {

// The k smallest (d2, index) keys of the candidates with d2 < bound, ascending, with their positions in the sorted array, in the last k of
// K slots (the first K - k hold key 0, which nothing undercuts, and never move: one instantiation serves every k <= K, and the pruning
// distance is the k-th best, not the K-th).  HeapExact's key (search.hpp); a slot that was never filled keeps position kNoIdx.  The
// interface of search.hpp's heaps.
template <int K_>
struct HeapNrm {
    static constexpr int K = K_;
    static constexpr bool kDeferred = false;
    uint64_t key[K];
    uint32_t pos[K];
    int k;
    uint32_t n_eval, n_shell;
    DCREG_DEVFN void init(float bound_f, float = 1.f, float = 0.f) {
        const uint64_t bound = (uint64_t)__float_as_uint(bound_f) << 32;      // index 0: d2 == bound does not enter
#pragma unroll
        for (int i = 0; i < K; ++i) { key[i] = i < K - k ? 0ull : bound; pos[i] = kNoIdx; }
        n_eval = 0; n_shell = 1;
    }
    DCREG_DEVFN void push(float d2, uint32_t idx, uint32_t p, bool valid = true) {
        const uint64_t kk = ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)idx;
        if (valid && kk < key[K - 1]) {
            key[K - 1] = kk; pos[K - 1] = p;
#pragma unroll
            for (int j = K - 1; j > 0; --j) {
                const bool sw = key[j] < key[j - 1];
                const uint64_t ka = key[j - 1], kb = key[j];
                const uint32_t pa = pos[j - 1], pb = pos[j];
                key[j - 1] = sw ? kb : ka; key[j] = sw ? ka : kb;
                pos[j - 1] = sw ? pb : pa; pos[j] = sw ? pa : pb;
            }
        }
    }
    DCREG_DEVFN float worst_d2() const { return __uint_as_float((uint32_t)(key[K - 1] >> 32)); }
};

}  // namespace dcreg
