// The Jacobi rotation that normals.hip and boxes.hip share: one step of the cyclic sweeps over a symmetric 3 x 3 matrix in
// fp64 (the numpy twin is randlanet/utils/normals.py: jacobi).  Only + - * / sqrt, each one correctly rounded: the files that
// include this are built with -ffp-contract=off.
#pragma once
#include "rl_common.h"

namespace {

// one rotation of the pair (p, q), r the third index: app, aqq, apq and the two off-diagonal entries arp, arq of the
// symmetric A, and the columns p and q of V.  A pair with apq == 0 is skipped by selects, so lanes do not diverge
// (the skipped lanes compute 0 / 0 and drop it).
__device__ __forceinline__ void nr_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                          double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    const bool skip = apq == 0.0;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double npp = app - t * apq, nqq = aqq + t * apq;
    const double nrp = c * arp - s * arq, nrq = s * arp + c * arq;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    app = skip ? app : npp; aqq = skip ? aqq : nqq;
    arp = skip ? arp : nrp; arq = skip ? arq : nrq;
    v0p = skip ? v0p : n0p; v0q = skip ? v0q : n0q;
    v1p = skip ? v1p : n1p; v1q = skip ? v1q : n1q;
    v2p = skip ? v2p : n2p; v2q = skip ? v2q : n2q;
    apq = 0.0;
}

}  // namespace
