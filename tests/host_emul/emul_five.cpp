// TEST INFRASTRUCTURE ONLY: host replay of the five-neighbour search of dcreg_amd/csrc/device/search.hpp (search5: HeapFast<5> behind the
// inclusive deferred filter, the boundary-tie test, the 64-bit-key search where it fires) on top of emul.cpp's index.
#include "emul.cpp"

extern "C" {

// search5 of host queries under the squared bound `bound` (strict), ring walk (sweep = 0) or row sweep (1, what k_lin runs): per query
// the five original indices (-1 where fewer lie inside the bound) and squared distances, in the order the search leaves them
int emu_search5(void *idx, const float *q_xyz, int64_t n, float bound, int sweep, int32_t *out_idx, float *out_d2) {
    EmuIndex *E = (EmuIndex *)idx;
    const GridDev &g = E->g;
    int kk = 1;
    while (kk < 100000) { const double s = (double)kk * g.h * (1.0 - 1e-9); if (s * s * (1.0 - 1e-6) >= (double)bound) break; ++kk; }
    static thread_local RunList runs;
    threadIdx.x = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float qx = q_xyz[3 * i], qy = q_xyz[3 * i + 1], qz = q_xyz[3 * i + 2];
        Set5 st;
        if (sweep) search5<true>(g, runs, qx, qy, qz, bound, kk, st);
        else search5<false>(g, runs, qx, qy, qz, bound, kk, st);
        for (int j = 0; j < 5; ++j) {
            const bool ok = st.pos[j] != kNoIdx;
            out_idx[5 * i + j] = ok ? (int32_t)__float_as_uint(g.pts[st.pos[j]].w) : -1;
            out_d2[5 * i + j] = ok ? st.d2[j] : INFINITY;
        }
    }
    return 0;
}

}  // extern "C"
