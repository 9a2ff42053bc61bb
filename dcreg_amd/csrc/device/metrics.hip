// calculatePointToPointError (DCReg/include/utils.hpp:538-589) on the device index:
//   forward  : every aligned source point (T * p, double arithmetic, float store as pcl::transformPointCloud
//              does for a Matrix4d) -> exact 1-NN in the target index; sum sqrt(d2), and d2 / count where
//              sqrt(d2) < error_threshold
//   backward : every target point -> 1-NN in the aligned cloud.  A rigid motion preserves distances, so the
//              nearest aligned point of q is the image of the nearest source point of T^-1 q; a second grid
//              index is built over the (body-frame) source once and queried with T^-1-transformed targets.
//              T^-1 is taken as (R^T, -R^T t): T must be a rigid motion, which the entry point checks on the host.
//              (The reference measures float distances between float-rounded aligned points, this pass between the
//              float-rounded T^-1 q and the source: the two means differ by rounding of 2^-24 of the largest
//              coordinate in each frame - the bound is stated in include/dcreg.h and asserted in tests/test_gpu_p2p_error.py.)
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg.h"
#include "context.hpp"

using namespace dcreg;

namespace dcreg {
int build_aux_index(dcreg_ctx *c);   // context.hip
}

static int reduce_p2p(dcreg_ctx *c, const float *d_d2, int64_t n, double thr, double out[3]) {
    const unsigned nb = (unsigned)((n + kBlock - 1) / kBlock);
    if (c->d_p2p_part.ensure(c, (size_t)nb * 4)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_p2p_partial, dim3(nb), dim3(kBlock), 0, c->stream, d_d2, n, thr, c->d_p2p_part.data());
    HIP_TRY(c, hipGetLastError());
    std::vector<double> h((size_t)nb * 4);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_p2p_part.data(), h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = 0.0;
    for (unsigned b = 0; b < nb; ++b) { out[0] += h[(size_t)b * 4]; out[1] += h[(size_t)b * 4 + 1]; out[2] += h[(size_t)b * 4 + 2]; }
    return DCREG_OK;
}

extern "C" int dcreg_p2p_error(dcreg_ctx *c, const double T[16], double error_threshold, double *rmse, double *fitness,
                               double *chamfer, int64_t *valid) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!T || !rmse || !fitness || !chamfer || !valid) { c->fail("null argument"); return DCREG_E_INVALID; }
    // the pose, on the host and before anything is queued or switched (the bottom row is ignored, as the reference's affine transform
    // ignores it): a non-finite entry would reach the cell arithmetic of the search, and the backward pass inverts T as a rigid motion
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) { c->fail("T has a non-finite entry"); return DCREG_E_INVALID; }
    if (!rigid_rotation(T)) { c->fail("the rotation block of T is not a rotation (|R^T R - I| > 1e-6 or det <= 0)"); return DCREG_E_INVALID; }
    (void)roi_deactivate(c);             // the metrics are taken on the whole map (context.hpp, the window index)
    if (c->map.n <= 0 || c->n_src <= 0) { c->fail("target / source clouds are not set"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t ns = c->n_src, nt = c->map.n;
    const int64_t nmax = ns > nt ? ns : nt;
    if (c->d_nn_idx.ensure(c, (size_t)nmax) || c->d_nn_d2.ensure(c, (size_t)nmax)) return DCREG_E_NOMEM;
    // forward: aligned -> target
    PoseArg P{};
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) P.R[i * 3 + j] = T[i * 4 + j]; P.t[i] = T[i * 4 + 3]; }
    int rc = launch_knn(c, c->map.grid, c->d_src_raw.data(), ns, 1, 0.0, &P, c->d_nn_idx.data(), c->d_nn_d2.data());
    if (rc) return rc;
    double fwd[3];
    rc = reduce_p2p(c, c->d_nn_d2.data(), ns, error_threshold, fwd);
    if (rc) return rc;
    // backward: target -> aligned  ==  T^-1 target -> source (body frame)
    rc = build_aux_index(c);
    if (rc) return rc;
    PoseArg Pi{};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Pi.R[i * 3 + j] = P.R[j * 3 + i];
        Pi.t[i] = -(P.R[0 * 3 + i] * P.t[0] + P.R[1 * 3 + i] * P.t[1] + P.R[2 * 3 + i] * P.t[2]);
    }
    rc = launch_knn(c, c->aux.grid, c->map.raw.data(), nt, 1, 0.0, &Pi, c->d_nn_idx.data(), c->d_nn_d2.data());
    if (rc) return rc;
    double bwd[3];
    rc = reduce_p2p(c, c->d_nn_d2.data(), nt, INFINITY, bwd);
    if (rc) return rc;
    *rmse = std::sqrt(fwd[1] / (double)ns);                               // utils.hpp:568
    *valid = (int64_t)std::llround(fwd[2]);
    *fitness = (double)*valid / (double)ns;                               // utils.hpp:572
    *chamfer = (fwd[0] / (double)ns + bwd[0] / (double)nt) / 2.0;         // utils.hpp:587
    return DCREG_OK;
}
