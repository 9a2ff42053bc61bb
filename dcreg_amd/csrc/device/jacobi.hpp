// The cyclic Jacobi rotation of the 3x3 eigen-solves (include/dcreg.h, "surface normals and curvature"): shared by the normals pass
// (normals.hip nrm_point) and the kept voxel map (voxel.hip k_vmap_reduce), which both run six sweeps of it over the pairs (0,1), (0,2), (1,2).
#pragma once
#include "search.hpp"

namespace dcreg {

// one Jacobi rotation of the pair (p, q), r the third index: the header's formulas, in its order
DCREG_DEVFN void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                            double &v1q, double &v2p, double &v2q) {
#pragma clang fp contract(off)
    double t = 0.0;
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    }
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tp = t * apq;
    app = app - tp;
    aqq = aqq + tp;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

}  // namespace dcreg
