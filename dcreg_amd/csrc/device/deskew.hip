// Motion compensation (deskew) of raw sweeps from per-point stamps (include/dcreg.h: dcreg_deskew*, dcreg_set_source_deskew*).  A spinning
// LiDAR measures each column of a sweep from a different sensor pose; under a constant twist xi = Log(motion) per cloud, point i moves by
// Exp(a_i xi) into the sensor frame at the reference instant (the exact rules are in the header).  No pass of its own over the records:
//   k_deskew_span   only for clouds with span_from_data - per cloud the minimum / maximum finite stamp (integer atomics on order-preserving
//                   64-bit keys: deterministic), read by the pack from the device (no readback)
//   k_pack_deskew   replaces k_pack inside upload_cloud: reads a record's x y z and stamp words, finds its cloud (seg_of), evaluates
//                   Exp(a xi) in fp64 and writes the packed float4 exactly as k_pack packs it (w = the point's index), or 3 floats
//   k_pack_deskew_path   the same pack for dcreg_deskew_path*: the pose at a point's stamp is read off a sampled trajectory (a binary search
//                   for its segment, Exp(u xi_k) along it) through a sensor-to-body extrinsic, from per-(cloud, segment) records the host
//                   prepares (deskew_path_prepare)
// Behind the pack everything runs as for a plain cloud - the voxel pass, the bounds, the source commit - so "bitwise the plain call of the
// deskewed cloud" holds by construction.  The call's counts ride on the readback the call has anyway.
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "context.hpp"
#include "../host/se3.hpp"

namespace dcreg {
namespace {

constexpr int kDskBlock = 256;
constexpr int kSpanPerThread = 8;                        // points per thread of k_deskew_span (a block covers one tile of 2048 points)
constexpr int kHead = 4;                                 // keys[0..3]: finite points, outside their span, minimum key, ~maximum key

// order-preserving key of a double (ascending keys = ascending values; -0.0 below +0.0) and its inverse
__device__ __forceinline__ unsigned long long key_of(double s) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(s);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double key_value(unsigned long long k) {
    union { unsigned long long u; double d; } cv;
    cv.u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return cv.d;
}

// s = scale * stamp, the stamp read from the record's raw words at `column` (64-bit types: column, column + 1, little-endian)
__device__ __forceinline__ double stamp_of(const float *__restrict__ rec, int column, int type, double scale) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(rec);
    const uint32_t lo = w[column];
    double v;
    if (type == DCREG_TIME_F32) {
        v = (double)__uint_as_float(lo);
    } else if (type == DCREG_TIME_U32) {
        v = (double)lo;
    } else {
        const uint32_t hi = w[column + 1];
        v = type == DCREG_TIME_F64 ? __hiloint2double((int)hi, (int)lo) : (double)(((unsigned long long)hi << 32) | lo);
    }
    return scale * v;
}

__device__ __forceinline__ void cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// q = R p + t with (R, t) = Exp(w, v) (se3.hpp se3Exp): R p = p + A w x p + B w x (w x p), t = v + B w x v + C w x (w x v)
__device__ __forceinline__ void exp_apply(const double w[3], const double v[3], const double p[3], double q[3]) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double A, B, Cc;
    if (th < 1e-3) {
        A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
        B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
        Cc = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
    } else {
        double s, c;
        sincos(th, &s, &c);
        A = s / th;
        B = (1.0 - c) / th2;
        Cc = (th - s) / (th2 * th);
    }
    double wp[3], wwp[3], wv[3], wwv[3];
    cross(w, p, wp); cross(w, wp, wwp);
    cross(w, v, wv); cross(w, wv, wwv);
    for (int a = 0; a < 3; ++a) q[a] = (p[a] + A * wp[a] + B * wwp[a]) + (v[a] + B * wv[a] + Cc * wwv[a]);
}

// the span of every span_from_data cloud: minimum key and ~maximum key of its finite stamps (points with finite x y z too).  A tile inside one
// cloud reduces in registers and LDS and adds 2 atomics; a tile across clouds adds per point.
static __global__ void __launch_bounds__(kDskBlock) k_deskew_span(const float *__restrict__ xyz, int64_t n, int64_t stride, int column, int type,
                                                                  double scale, const int64_t *__restrict__ off, int n_clouds,
                                                                  const DeskewCloud *__restrict__ cl, unsigned long long *__restrict__ keys) {
    const int64_t base = (int64_t)blockIdx.x * (kDskBlock * kSpanPerThread);
    const int64_t last = std::min<int64_t>(n, base + kDskBlock * kSpanPerThread) - 1;
    const uint32_t s0 = seg_of(off, n_clouds, base);
    const bool uniform = seg_of(off, n_clouds, last) == s0;
    if (uniform && !cl[s0].from_data) return;           // (block-uniform)
    unsigned long long kmin = ~0ull, kmaxn = ~0ull;
    for (int k = 0; k < kSpanPerThread; ++k) {
        const int64_t i = base + threadIdx.x + (int64_t)k * kDskBlock;
        if (i > last) break;
        const uint32_t s = uniform ? s0 : seg_of(off, n_clouds, i);
        if (!cl[s].from_data) continue;
        const float *r = xyz + i * stride;
        const double t = stamp_of(r, column, type, scale);
        if (!finite_xyz(r[0], r[1], r[2]) || !isfinite(t)) continue;
        const unsigned long long kk = key_of(t);
        if (uniform) {
            kmin = std::min(kmin, kk); kmaxn = std::min(kmaxn, ~kk);
        } else {
            atomicMin(keys + kHead + 2 * s, kk);
            atomicMin(keys + kHead + 2 * s + 1, ~kk);
        }
    }
    if (!uniform) return;          // (block-uniform)
    for (int o = 32; o > 0; o >>= 1) {
        kmin = std::min(kmin, (unsigned long long)__shfl_xor(kmin, o));
        kmaxn = std::min(kmaxn, (unsigned long long)__shfl_xor(kmaxn, o));
    }
    __shared__ unsigned long long smin[kDskBlock / 64], smaxn[kDskBlock / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smin[wave] = kmin; smaxn[wave] = kmaxn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDskBlock / 64; ++w) { kmin = std::min(kmin, smin[w]); kmaxn = std::min(kmaxn, smaxn[w]); }
        if (kmin != ~0ull) {
            atomicMin(keys + kHead + 2 * s0, kmin);
            atomicMin(keys + kHead + 2 * s0 + 1, kmaxn);
        }
    }
}

// the tail both pack kernels share.  pack_store: point i as k_pack packs a record (w = the point's index), or 3 floats
__device__ __forceinline__ void pack_store(float4 *__restrict__ out4, float *__restrict__ out3, int64_t i, float ox, float oy, float oz) {
    if (out4) out4[i] = make_float4(ox, oy, oz, __uint_as_float((uint32_t)i));
    else { out3[3 * i] = ox; out3[3 * i + 1] = oy; out3[3 * i + 2] = oz; }
}
// reduce_counts: a lane's counts (finite, outside its span, its stamp's key and ~key) reduce per wave, then per block, into keys[0..3].  Every
// thread of the block calls it
__device__ __forceinline__ void reduce_counts(unsigned long long fin, unsigned long long outside, unsigned long long kmin,
                                              unsigned long long kmaxn, unsigned long long *__restrict__ keys) {
    for (int o = 32; o > 0; o >>= 1) {
        fin += __shfl_xor(fin, o);
        outside += __shfl_xor(outside, o);
        kmin = std::min(kmin, (unsigned long long)__shfl_xor(kmin, o));
        kmaxn = std::min(kmaxn, (unsigned long long)__shfl_xor(kmaxn, o));
    }
    __shared__ unsigned long long sh[kDskBlock / 64][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave][0] = fin; sh[wave][1] = outside; sh[wave][2] = kmin; sh[wave][3] = kmaxn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDskBlock / 64; ++w) {
            fin += sh[w][0]; outside += sh[w][1];
            kmin = std::min(kmin, sh[w][2]); kmaxn = std::min(kmaxn, sh[w][3]);
        }
        if (fin) {
            atomicAdd(keys, fin);
            if (outside) atomicAdd(keys + 1, outside);
            atomicMin(keys + 2, kmin);
            atomicMin(keys + 3, kmaxn);
        }
    }
}

// the pack of a deskewed cloud: out4[i] = (x', y', z', i) as k_pack packs a record, or out3[3i ..] = x', y', z'.  One point per lane; the call's
// counts (finite points, stamps outside their span, minimum / maximum finite stamp) reduce per block into keys[0..3]
static __global__ void __launch_bounds__(kDskBlock) k_pack_deskew(const float *__restrict__ xyz, int64_t n, int64_t stride, int column, int type,
                                                                  double scale, const int64_t *__restrict__ off, int n_clouds,
                                                                  const DeskewCloud *__restrict__ cl, unsigned long long *__restrict__ keys,
                                                                  float4 *__restrict__ out4, float *__restrict__ out3) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long fin = 0, outside = 0, kmin = ~0ull, kmaxn = ~0ull;
    if (i < n) {
        const float *r = xyz + i * stride;
        const float x = r[0], y = r[1], z = r[2];
        const double t = stamp_of(r, column, type, scale);
        float ox = __builtin_nanf(""), oy = ox, oz = ox;
        if (finite_xyz(x, y, z) && isfinite(t)) {
            const uint32_t s = n_clouds == 1 ? 0u : seg_of(off, n_clouds, i);
            const DeskewCloud &q = cl[s];
            double tb = q.t_begin, te = q.t_end;
            if (q.from_data) {         // (this point is finite: its cloud's keys hold a span)
                tb = key_value(keys[kHead + 2 * s]);
                te = key_value(~keys[kHead + 2 * s + 1]);
            }
            const double len = te - tb;
            const double al = len > 0.0 ? (t - tb) / len - q.ref : 0.0;
            const double w[3] = {al * q.xi[0], al * q.xi[1], al * q.xi[2]}, v[3] = {al * q.xi[3], al * q.xi[4], al * q.xi[5]};
            if (w[0] == 0.0 && w[1] == 0.0 && w[2] == 0.0 && v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0) {
                ox = x; oy = y; oz = z;            // a_i xi = 0: the point bit for bit (-0.0 stays -0.0)
            } else {
                const double p[3] = {(double)x, (double)y, (double)z};
                double o[3];
                exp_apply(w, v, p, o);
                ox = (float)o[0]; oy = (float)o[1]; oz = (float)o[2];
            }
            fin = 1;
            outside = (t < tb || t > te) ? 1 : 0;
            kmin = key_of(t);
            kmaxn = ~kmin;
        }
        pack_store(out4, out3, i, ox, oy, oz);
    }
    reduce_counts(fin, outside, kmin, kmaxn, keys);
}

// q = R p + t for a rigid transform stored as R[9] row-major then t[3]
__device__ __forceinline__ void rigid_apply(const double *__restrict__ T, const double p[3], double q[3]) {
    for (int a = 0; a < 3; ++a) q[a] = (T[3 * a] * p[0] + T[3 * a + 1] * p[1] + T[3 * a + 2] * p[2]) + T[9 + a];
}

// the pack of a cloud deskewed along its path (dcreg_deskew_path*): the point's cloud by seg_of, its segment by a binary search over the
// starts of the cloud's segment records (the last one that starts at or before the stamp; the first for an earlier stamp), then q = E p,
// q = Exp(u xi_k) q, p' = G_k q.  Lanes of a wave are neighbouring columns of a sweep: they read the same or neighbouring records.  Output
// and counts as k_pack_deskew
static __global__ void __launch_bounds__(kDskBlock) k_pack_deskew_path(const float *__restrict__ xyz, int64_t n, int64_t stride, int column, int type,
                                                                       double scale, const int64_t *__restrict__ off, int n_clouds,
                                                                       const PathCloud *__restrict__ cl, const PathSeg *__restrict__ sg,
                                                                       unsigned long long *__restrict__ keys, float4 *__restrict__ out4,
                                                                       float *__restrict__ out3) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long fin = 0, outside = 0, kmin = ~0ull, kmaxn = ~0ull;
    if (i < n) {
        const float *r = xyz + i * stride;
        const float x = r[0], y = r[1], z = r[2];
        const double t = stamp_of(r, column, type, scale);
        float ox = __builtin_nanf(""), oy = ox, oz = ox;
        if (finite_xyz(x, y, z) && isfinite(t)) {
            const uint32_t s = n_clouds == 1 ? 0u : seg_of(off, n_clouds, i);
            const PathCloud &q = cl[s];
            const PathSeg *S = sg + q.first_seg;
            int lo = 0, hi = q.n_seg - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (S[mid].s0 <= t) lo = mid; else hi = mid - 1;
            }
            const PathSeg &g = S[lo];
            const double u = (t - g.s0) / g.len;
            const double w[3] = {u * g.xi[0], u * g.xi[1], u * g.xi[2]}, v[3] = {u * g.xi[3], u * g.xi[4], u * g.xi[5]};
            const double p[3] = {(double)x, (double)y, (double)z};
            double a[3], b[3], o[3];
            rigid_apply(q.E, p, a);
            exp_apply(w, v, a, b);
            rigid_apply(g.G, b, o);
            ox = (float)o[0]; oy = (float)o[1]; oz = (float)o[2];
            fin = 1;
            outside = (t < q.s_first || t > q.s_last) ? 1 : 0;
            kmin = key_of(t);
            kmaxn = ~kmin;
        }
        pack_store(out4, out3, i, ox, oy, oz);
    }
    reduce_counts(fin, outside, kmin, kmaxn, keys);
}

bool is_rotation(const double R[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0);   // (R^T R - I)_ij
            if (!(std::fabs(g) <= 1e-6)) return false;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return det > 0.0;
}

}  // namespace

// what both forms check of the clouds and the time field (blocks: the per-cloud motions or path blocks are there)
static int check_clouds_and_field(dcreg_ctx *c, int n_clouds, const int64_t *off, int64_t stride, const dcreg_time_field *f, bool blocks) {
    if (!f) { c->fail("null time field"); return DCREG_E_INVALID; }
    if (n_clouds < 0 || (n_clouds > 0 && (!off || !blocks)) || stride < 3) { c->fail("invalid cloud arguments"); return DCREG_E_INVALID; }
    if (n_clouds > 0 && off[0] != 0) { c->fail("cloud offsets must start at 0"); return DCREG_E_INVALID; }
    for (int s = 0; s < n_clouds; ++s)
        if (off[s + 1] < off[s]) { c->fail("cloud offsets decrease at cloud %d", s); return DCREG_E_INVALID; }
    if (f->type < DCREG_TIME_F32 || f->type > DCREG_TIME_U64) { c->fail("unknown time type %d", f->type); return DCREG_E_INVALID; }
    const bool wide = f->type == DCREG_TIME_F64 || f->type == DCREG_TIME_U64;
    if (f->column < 3 || f->column >= stride || (wide && (int64_t)f->column + 1 >= stride)) {
        c->fail("time column %d outside [3, %lld)%s", f->column, (long long)stride, wide ? " (a 64-bit stamp takes two slots)" : "");
        return DCREG_E_INVALID;
    }
    if (!(std::isfinite(f->scale) && f->scale > 0.0)) { c->fail("time scale %g: finite and > 0 expected", f->scale); return DCREG_E_INVALID; }
    return DCREG_OK;
}

static void run_of(DeskewRun &d, int n_clouds, const int64_t *off, const dcreg_time_field *f) {
    d.n_clouds = n_clouds;
    d.off = off;
    d.column = f->column;
    d.type = f->type;
    d.scale = f->scale;
}

int deskew_prepare(dcreg_ctx *c, int n_clouds, const int64_t *off, int64_t stride, const dcreg_time_field *f, const dcreg_sweep_motion *m,
                   DeskewRun &d) {
    if (int rc = check_clouds_and_field(c, n_clouds, off, stride, f, m != nullptr)) return rc;
    d = DeskewRun();
    d.clouds.resize((size_t)n_clouds);
    for (int s = 0; s < n_clouds; ++s) {
        const dcreg_sweep_motion &q = m[s];
        bool finite = true;
        for (int k = 0; k < 9; ++k) finite &= std::isfinite(q.R[k]);
        for (int k = 0; k < 3; ++k) finite &= std::isfinite(q.t[k]);
        if (!finite) { c->fail("cloud %d: the motion is not finite", s); return DCREG_E_INVALID; }
        if (!is_rotation(q.R)) { c->fail("cloud %d: R is not a rotation (|R^T R - I| > 1e-6 or det <= 0)", s); return DCREG_E_INVALID; }
        if (!q.span_from_data && !(std::isfinite(q.t_begin) && std::isfinite(q.t_end) && q.t_end >= q.t_begin)) {
            c->fail("cloud %d: span [%g, %g] is not finite and ordered", s, q.t_begin, q.t_end);
            return DCREG_E_INVALID;
        }
        if (!(q.ref >= 0.0 && q.ref <= 1.0)) { c->fail("cloud %d: ref %g outside [0, 1]", s, q.ref); return DCREG_E_INVALID; }
        DeskewCloud &o = d.clouds[(size_t)s];
        const double th = se3Log(q.R, q.t, o.xi);
        if (!(th < M_PI / 2)) { c->fail("cloud %d: the motion rotates by %g rad (below pi/2 expected)", s, th); return DCREG_E_INVALID; }
        o.t_begin = q.span_from_data ? 0.0 : q.t_begin;
        o.t_end = q.span_from_data ? 0.0 : q.t_end;
        o.ref = q.ref;
        o.from_data = q.span_from_data ? 1 : 0;
        o.pad_ = 0;
        d.any_from_data |= o.from_data != 0;
    }
    run_of(d, n_clouds, off, f);
    return DCREG_OK;
}

// C = A^T B of two rotations; o = A^T v
static void mat3tmul(const double *A, const double *B, double *C) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
static void mat3tvec(const double *A, const double v[3], double o[3]) {
    for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}

// the path form: every refusal of include/dcreg.h, then per (cloud, segment) the twist xi_k and G_k = E^-1 B(t_ref)^-1 P_k in double.  A knot
// and a segment of the table are checked (and the segment's twist taken) once per call, however many windows hold them.
int deskew_path_prepare(dcreg_ctx *c, int n_clouds, const int64_t *off, int64_t stride, const dcreg_time_field *f, const PathTable &t,
                        DeskewRun &d) {
    if (int rc = check_clouds_and_field(c, n_clouds, off, stride, f, t.paths != nullptr)) return rc;
    if (n_clouds > 0 && (t.n_knots < 0 || !t.stamps || !t.poses)) { c->fail("null knot table"); return DCREG_E_INVALID; }
    d = DeskewRun();
    d.path = true;
    d.pclouds.resize((size_t)n_clouds);
    int64_t n_seg = 0;
    for (int s = 0; s < n_clouds; ++s) {
        const dcreg_sweep_path &q = t.paths[s];
        if (q.n_knots < 2 || q.first_knot < 0 || q.first_knot > t.n_knots || (int64_t)q.n_knots > t.n_knots - q.first_knot) {
            c->fail("cloud %d: the window of %d knots from %lld is outside the table of %lld knots or has fewer than 2 knots", s, q.n_knots,
                    (long long)q.first_knot, (long long)t.n_knots);
            return DCREG_E_INVALID;
        }
        n_seg += q.n_knots - 1;
    }
    d.segs.resize((size_t)n_seg);
    int64_t k_lo = t.n_knots, k_hi = 0;              // the knots some window holds lie in [k_lo, k_hi)
    for (int s = 0; s < n_clouds; ++s) {
        k_lo = std::min(k_lo, t.paths[s].first_knot);
        k_hi = std::max(k_hi, t.paths[s].first_knot + t.paths[s].n_knots);
    }
    std::vector<char> knot_ok((size_t)std::max<int64_t>(k_hi - k_lo, 0), 0), seg_ok(knot_ok.size(), 0);
    std::vector<double> xis(6 * knot_ok.size());
    n_seg = 0;
    for (int s = 0; s < n_clouds; ++s) {
        const dcreg_sweep_path &q = t.paths[s];
        const int K = q.n_knots;
        const double *st = t.stamps + q.first_knot, *P = t.poses + 12 * q.first_knot;
        for (int k = 0; k < K; ++k) {
            const int64_t j = q.first_knot + k, jj = j - k_lo;
            if (!knot_ok[(size_t)jj]) {
                if (!finite_n(P + 12 * k, 12)) { c->fail("cloud %d: the pose of knot %lld is not finite", s, (long long)j); return DCREG_E_INVALID; }
                if (!is_rotation(P + 12 * k)) {
                    c->fail("cloud %d: R of knot %lld is not a rotation (|R^T R - I| > 1e-6 or det <= 0)", s, (long long)j);
                    return DCREG_E_INVALID;
                }
                knot_ok[(size_t)jj] = 1;
            }
            if (!std::isfinite(st[k]) || (k > 0 && !(st[k] > st[k - 1]))) {
                c->fail("cloud %d: the stamps of its knots are not finite and strictly increasing at knot %lld", s, (long long)j);
                return DCREG_E_INVALID;
            }
            if (k > 0 && !seg_ok[(size_t)jj - 1]) {
                const double *A = P + 12 * (k - 1), *B = P + 12 * k;
                const double dt[3] = {B[9] - A[9], B[10] - A[10], B[11] - A[11]};
                double R[9], tt[3];
                mat3tmul(A, B, R);
                mat3tvec(A, dt, tt);
                const double th = se3Log(R, tt, &xis[6 * ((size_t)jj - 1)]);
                if (!(th < M_PI / 2)) {
                    c->fail("cloud %d: the segment before knot %lld rotates by %g rad (below pi/2 expected)", s, (long long)j, th);
                    return DCREG_E_INVALID;
                }
                seg_ok[(size_t)jj - 1] = 1;
            }
        }
        if (!finite_n(q.ext_R, 9) || !finite_n(q.ext_t, 3)) { c->fail("cloud %d: the extrinsic is not finite", s); return DCREG_E_INVALID; }
        if (!is_rotation(q.ext_R)) { c->fail("cloud %d: the extrinsic's R is not a rotation (|R^T R - I| > 1e-6 or det <= 0)", s); return DCREG_E_INVALID; }
        if (!(std::isfinite(q.t_ref) && q.t_ref >= st[0] && q.t_ref <= st[K - 1])) {
            c->fail("cloud %d: t_ref %.17g outside its knots' [%.17g, %.17g]", s, q.t_ref, st[0], st[K - 1]);
            return DCREG_E_INVALID;
        }
        int kr = 0;                                    // B(t_ref) = P_kr Exp(ur xi_kr) = (Rb, P_kr.t + P_kr.R tb)
        for (int j = 1; j <= K - 2; ++j) kr += st[j] <= q.t_ref ? 1 : 0;
        const double ur = (q.t_ref - st[kr]) / (st[kr + 1] - st[kr]);
        const double *xr = &xis[6 * (size_t)(q.first_knot - k_lo + kr)], *Pr = P + 12 * kr;
        const double xu[6] = {ur * xr[0], ur * xr[1], ur * xr[2], ur * xr[3], ur * xr[4], ur * xr[5]};
        double Re[9], te[3], Rb[9], tb[3];
        se3Exp(xu, Re, te);
        mat3mul(Pr, Re, Rb);
        for (int a = 0; a < 3; ++a) tb[a] = Pr[3 * a] * te[0] + Pr[3 * a + 1] * te[1] + Pr[3 * a + 2] * te[2];
        PathCloud &o = d.pclouds[(size_t)s];
        o.first_seg = n_seg;
        o.n_seg = K - 1;
        o.pad_ = 0;
        o.s_first = st[0];
        o.s_last = st[K - 1];
        std::memcpy(o.E, q.ext_R, sizeof(q.ext_R));
        std::memcpy(o.E + 9, q.ext_t, sizeof(q.ext_t));
        for (int k = 0; k < K - 1; ++k) {
            PathSeg &g = d.segs[(size_t)(n_seg + k)];
            std::memcpy(g.xi, &xis[6 * (size_t)(q.first_knot - k_lo + k)], sizeof(g.xi));
            const double *Pk = P + 12 * k;
            double M[9], dk[3], tm[3];                 // B(t_ref)^-1 P_k = (Rb^T R_k, Rb^T ((t_k - t_kr) - tb))
            mat3tmul(Rb, Pk, M);
            for (int a = 0; a < 3; ++a) dk[a] = (Pk[9 + a] - Pr[9 + a]) - tb[a];
            mat3tvec(Rb, dk, tm);
            for (int a = 0; a < 3; ++a) tm[a] -= q.ext_t[a];
            mat3tmul(q.ext_R, M, g.G);                 // E^-1 (M, tm) = (E_R^T M, E_R^T (tm - E_t))
            mat3tvec(q.ext_R, tm, g.G + 9);
            g.s0 = st[k];
            g.len = st[k + 1] - st[k];
        }
        n_seg += K - 1;
    }
    run_of(d, n_clouds, off, f);
    return DCREG_OK;
}

int deskew_reserve(dcreg_ctx *c, const DeskewRun &d) {
    dcreg_ctx::DeskewBufs &B = c->dsk;
    if (B.d_off.ensure(c, (size_t)d.n_clouds + 1) || B.keys.ensure(c, (size_t)kHead + 2 * (size_t)d.n_clouds)) return DCREG_E_NOMEM;
    if (d.path ? B.pclouds.ensure(c, d.pclouds.size()) || B.segs.ensure(c, d.segs.size()) : B.clouds.ensure(c, (size_t)d.n_clouds)) return DCREG_E_NOMEM;
    return DCREG_OK;
}

int deskew_queue(dcreg_ctx *c, const float *src, int64_t n, int64_t stride, DeskewRun &d, float4 *out4) {
    dcreg_ctx::DeskewBufs &B = c->dsk;
    const size_t nk = (size_t)kHead + 2 * (size_t)d.n_clouds;
    if (d.path) {
        HIP_TRY(c, hipMemcpyAsync(B.pclouds.data(), d.pclouds.data(), sizeof(PathCloud) * d.pclouds.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(B.segs.data(), d.segs.data(), sizeof(PathSeg) * d.segs.size(), hipMemcpyHostToDevice, c->stream));
    } else {
        HIP_TRY(c, hipMemcpyAsync(B.clouds.data(), d.clouds.data(), sizeof(DeskewCloud) * d.clouds.size(), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(B.d_off.data(), d.off, sizeof(int64_t) * ((size_t)d.n_clouds + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(B.keys.data(), 0, 2 * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(B.keys.data() + 2, 0xFF, (nk - 2) * sizeof(unsigned long long), c->stream));
    if (d.any_from_data)
        hipLaunchKernelGGL(k_deskew_span, dim3(blocks(n, kDskBlock * kSpanPerThread)), dim3(kDskBlock), 0, c->stream, src, n, stride, d.column, d.type,
                           d.scale, B.d_off.data(), d.n_clouds, B.clouds.data(), B.keys.data());
    if (d.path)
        hipLaunchKernelGGL(k_pack_deskew_path, dim3(blocks(n, kDskBlock)), dim3(kDskBlock), 0, c->stream, src, n, stride, d.column, d.type, d.scale,
                           B.d_off.data(), d.n_clouds, B.pclouds.data(), B.segs.data(), B.keys.data(), out4, d.out3);
    else
        hipLaunchKernelGGL(k_pack_deskew, dim3(blocks(n, kDskBlock)), dim3(kDskBlock), 0, c->stream, src, n, stride, d.column, d.type, d.scale,
                           B.d_off.data(), d.n_clouds, B.clouds.data(), B.keys.data(), out4, d.out3);
    HIP_TRY(c, hipGetLastError());
    d.queued = true;
    return DCREG_OK;
}

int deskew_readback(dcreg_ctx *c, DeskewRun &d) {
    if (!d.queued) return DCREG_OK;
    HIP_TRY(c, hipMemcpyAsync(d.head, c->dsk.keys.data(), sizeof(d.head), hipMemcpyDeviceToHost, c->stream));
    d.read = true;
    return DCREG_OK;
}

void deskew_info(const DeskewRun &d, int64_t n_in, dcreg_deskew_info *info) {
    if (!info) return;
    const bool any = d.read && d.head[0] > 0;
    info->n_in = n_in;
    info->n_finite = any ? (int64_t)d.head[0] : 0;
    info->n_outside = any ? (int64_t)d.head[1] : 0;
    info->t_min = any ? key_value(d.head[2]) : NAN;
    info->t_max = any ? key_value(~d.head[3]) : NAN;
}

}  // namespace dcreg

using namespace dcreg;

// dcreg_deskew*: with a voxel block the voxel pass of the deskewed clouds (voxel.hip); without one every point in input order, written by the
// pack itself (to the caller's device buffer, or to the context's and copied to the host with the counts)
// (pt: the path form, dcreg_deskew_path*; m otherwise)
static int deskew(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, const dcreg_time_field *f,
                  const dcreg_sweep_motion *m, const PathTable *pt, const dcreg_voxel_params *voxel, float *out, int64_t capacity,
                  int64_t *out_off, dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    DeskewRun d;
    int rc = pt ? deskew_path_prepare(c, n_clouds, off, stride, f, *pt, d) : deskew_prepare(c, n_clouds, off, stride, f, m, d);
    if (rc) return rc;
    const int64_t n = n_clouds > 0 ? off[n_clouds] : 0;
    if (voxel) {
        rc = voxel_downsample_to(c, n_clouds, xyz, off, stride, on_device, voxel, out, capacity, out_off, vinfo, &d);
        if (rc == DCREG_OK || d.read) deskew_info(d, n, info);
        return rc;
    }
    if (!out_off || capacity < 0) { c->fail("invalid output arguments"); return DCREG_E_INVALID; }
    out_off[0] = 0;
    for (int s = 1; s <= n_clouds; ++s) out_off[s] = off[s];
    if (n > capacity) { c->fail("the output holds %lld points, the capacity is %lld", (long long)n, (long long)capacity); return DCREG_E_INVALID; }
    if (n == 0) { deskew_info(d, 0, info); return DCREG_OK; }
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (!on_device && c->vox.out.ensure(c, (size_t)(3 * n))) return DCREG_E_NOMEM;
    d.out3 = on_device ? out : c->vox.out.data();
    rc = upload_cloud(c, xyz, n, stride, on_device, c->vox.pts, &d);
    if (rc) return rc;
    if ((rc = deskew_readback(c, d))) return rc;
    if (!on_device) HIP_TRY(c, hipMemcpyAsync(out, c->vox.out.data(), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    deskew_info(d, n, info);
    return DCREG_OK;
}

extern "C" {
int dcreg_deskew(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_time_field *f,
                 const dcreg_sweep_motion *motions, const dcreg_voxel_params *voxel, float *out_xyz, int64_t capacity_points, int64_t *out_offsets,
                 dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    return deskew(c, n_clouds, xyz, offsets, stride_floats, false, f, motions, nullptr, voxel, out_xyz, capacity_points, out_offsets, info, vinfo);
}
int dcreg_deskew_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_time_field *f,
                        const dcreg_sweep_motion *motions, const dcreg_voxel_params *voxel, float *d_out_xyz, int64_t capacity_points,
                        int64_t *out_offsets, dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    return deskew(c, n_clouds, d_xyz, offsets, stride_floats, true, f, motions, nullptr, voxel, d_out_xyz, capacity_points, out_offsets, info, vinfo);
}
int dcreg_deskew_path(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_time_field *f,
                      int64_t n_knots, const double *knot_stamps, const double *knot_poses, const dcreg_sweep_path *paths,
                      const dcreg_voxel_params *voxel, float *out_xyz, int64_t capacity_points, int64_t *out_offsets, dcreg_deskew_info *info,
                      dcreg_voxel_info *vinfo) {
    const PathTable pt = {n_knots, knot_stamps, knot_poses, paths};
    return deskew(c, n_clouds, xyz, offsets, stride_floats, false, f, nullptr, &pt, voxel, out_xyz, capacity_points, out_offsets, info, vinfo);
}
int dcreg_deskew_path_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                             const dcreg_time_field *f, int64_t n_knots, const double *knot_stamps, const double *knot_poses,
                             const dcreg_sweep_path *paths, const dcreg_voxel_params *voxel, float *d_out_xyz, int64_t capacity_points,
                             int64_t *out_offsets, dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    const PathTable pt = {n_knots, knot_stamps, knot_poses, paths};
    return deskew(c, n_clouds, d_xyz, offsets, stride_floats, true, f, nullptr, &pt, voxel, d_out_xyz, capacity_points, out_offsets, info, vinfo);
}
}
