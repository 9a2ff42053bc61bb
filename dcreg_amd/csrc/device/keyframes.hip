// Keyframe store and submaps on the device (include/dcreg.h: dcreg_keyframes_*, dcreg_set_target_keyframes).
// The clouds a mapper registers are kept where they already are - in device memory, 3 floats per point, bit for bit - and a submap (an
// ordered list of (keyframe id, pose) members) is assembled from them by ONE kernel:
//   k_kf_store     an added cloud (packed by upload_cloud, or the context's source in input order) -> the store; flags a non-finite point
//   k_kf_gather    the gather-transform pack: output point i of a call belongs to the member whose output start is the largest <= i; its
//                  stored point is moved by the member's pose (search.hpp body_to_global's rule) and written as the float4 record
//                  k_pack writes (into the voxel pass or the target build: upload_cloud's GatherRun hook) or as 3 floats per point
// A block owns a tile of kKfBlock x kKfPerThread consecutive OUTPUT points, as k_vox_coords owns its tile.  A tile inside one member reads
// that member's record once (block-uniform) and streams; a tile across members finds every point's member by binary search.
// Poses are arguments of every call and never stored; nothing is composed on the host, so the 12 numbers given fix every output bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "context.hpp"

namespace dcreg {
namespace {

constexpr int kKfBlock = 256;
constexpr int kKfPerThread = 8;                          // output points per thread (a block covers one tile of 2048 points)
constexpr int kKfTile = kKfBlock * kKfPerThread;
constexpr int64_t kKfMaxStored = ((int64_t)1 << 32) - 1;  // points the store may hold (KfMember::src is 32 bits wide: 51.5 GB of points)
constexpr int64_t kKfMaxCall = ((int64_t)1 << 31) - 1;    // a call gathers fewer member points than this (the voxel pass's limit)

// the member of output point i: the largest m with mem[m].start <= i (the starts ascend strictly: empty members are not in the list)
__device__ __forceinline__ int member_of(const KfMember *__restrict__ mem, int n_members, uint32_t i) {
    int lo = 0, hi = n_members - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mem[mid].start <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// q_a = (float)(R[a][0] p_x + R[a][1] p_y + R[a][2] p_z + t[a]) in double, left to right, every product and sum rounded (no contraction):
// search.hpp body_to_global, the transform of dcreg_target_insert
__device__ __forceinline__ void kf_move(const double *__restrict__ P, float px, float py, float pz, float &qx, float &qy, float &qz) {
#pragma clang fp contract(off)
    const double x = (double)px, y = (double)py, z = (double)pz;
    qx = (float)(P[0] * x + P[1] * y + P[2] * z + P[9]);
    qy = (float)(P[3] * x + P[4] * y + P[5] * z + P[10]);
    qz = (float)(P[6] * x + P[7] * y + P[8] * z + P[11]);
}

// The gather-transform pack.  OUT3 false: out4[i] = (q, w = i) as k_pack writes a cloud; OUT3 true: 3 floats per point to out3 - a lane
// of a tile inside one member then takes 4 consecutive points and writes them as three 16-byte stores where out3 is 16-byte aligned (vec3).
template <bool OUT3>
static __global__ void __launch_bounds__(kKfBlock) k_kf_gather(const float *__restrict__ store, const KfMember *__restrict__ mem, int n_members,
                                                               int64_t n, float4 *__restrict__ out4, float *__restrict__ out3, int vec3) {
    const int64_t base = (int64_t)blockIdx.x * kKfTile;
    const int64_t last = std::min<int64_t>(n, base + kKfTile) - 1;
    const int m0 = member_of(mem, n_members, (uint32_t)base);
    const bool uniform = member_of(mem, n_members, (uint32_t)last) == m0;
    if (uniform) {                 // (block-uniform) the member's record once, then 12-byte records, consecutive lanes adjacent
        double P[12];
        for (int e = 0; e < 12; ++e) P[e] = mem[m0].pose[e];
        const float *__restrict__ src = store + 3 * ((int64_t)mem[m0].src + (base - (int64_t)mem[m0].start));     // the record of point `base`
        if constexpr (OUT3) {
            for (int k = 0; k < kKfPerThread / 4; ++k) {
                const int64_t j = 4 * ((int64_t)threadIdx.x + (int64_t)k * kKfBlock);      // first of the lane's 4 points, within the tile
                if (base + j > last) break;
                if (vec3 && base + j + 3 <= last) {
                    float q[12];
                    for (int u = 0; u < 4; ++u) {
                        const float *p = src + 3 * (j + u);
                        kf_move(P, p[0], p[1], p[2], q[3 * u], q[3 * u + 1], q[3 * u + 2]);
                    }
                    float4 *o = reinterpret_cast<float4 *>(out3 + 3 * (base + j));
                    o[0] = make_float4(q[0], q[1], q[2], q[3]);
                    o[1] = make_float4(q[4], q[5], q[6], q[7]);
                    o[2] = make_float4(q[8], q[9], q[10], q[11]);
                } else {
                    for (int64_t u = j; u < j + 4 && base + u <= last; ++u) {
                        float qx, qy, qz;
                        kf_move(P, src[3 * u], src[3 * u + 1], src[3 * u + 2], qx, qy, qz);
                        float *o = out3 + 3 * (base + u);
                        o[0] = qx; o[1] = qy; o[2] = qz;
                    }
                }
            }
        } else {
            for (int k = 0; k < kKfPerThread; ++k) {
                const int64_t j = (int64_t)threadIdx.x + (int64_t)k * kKfBlock;
                if (base + j > last) break;
                float qx, qy, qz;
                kf_move(P, src[3 * j], src[3 * j + 1], src[3 * j + 2], qx, qy, qz);
                out4[base + j] = make_float4(qx, qy, qz, __uint_as_float((uint32_t)(base + j)));
            }
        }
        return;
    }
    for (int k = 0; k < kKfPerThread; ++k) {       // a tile across members: every point finds its own
        const int64_t i = base + threadIdx.x + (int64_t)k * kKfBlock;
        if (i > last) break;
        const KfMember *__restrict__ M = mem + member_of(mem, n_members, (uint32_t)i);
        const float *__restrict__ p = store + 3 * ((int64_t)M->src + (i - (int64_t)M->start));
        float qx, qy, qz;
        kf_move(M->pose, p[0], p[1], p[2], qx, qy, qz);
        if constexpr (OUT3) {
            float *o = out3 + 3 * i;
            o[0] = qx; o[1] = qy; o[2] = qz;
        } else {
            out4[i] = make_float4(qx, qy, qz, __uint_as_float((uint32_t)i));
        }
    }
}

// n packed points (k_pack's records) -> 3 floats each at out, bit for bit; *flag |= 1 when a coordinate is not finite
static __global__ void k_kf_store(const float4 *__restrict__ in, int64_t n, float *__restrict__ out, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    out[3 * i] = p.x; out[3 * i + 1] = p.y; out[3 * i + 2] = p.z;
    if (!finite_point(p)) atomicOr(flag, 1u);
}

// what every entry point does first
int enter(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return DCREG_OK;
}

int check_ready(dcreg_ctx *c) {
    if (!c->kf.ready) { c->fail("no keyframe store: dcreg_keyframes_reset first"); return DCREG_E_STATE; }
    return DCREG_OK;
}

int check_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride) {
    if (n_clouds < 0 || (n_clouds > 0 && !off) || stride < 3) { c->fail("invalid cloud arguments"); return DCREG_E_INVALID; }
    if (n_clouds > 0 && off[0] != 0) { c->fail("cloud offsets must start at 0"); return DCREG_E_INVALID; }
    for (int s = 0; s < n_clouds; ++s)
        if (off[s + 1] < off[s]) { c->fail("cloud offsets decrease at cloud %d", s); return DCREG_E_INVALID; }
    const int64_t n = n_clouds > 0 ? off[n_clouds] : 0;
    if (n >= kKfMaxCall) { c->fail("too many points for one call (%lld)", (long long)n); return DCREG_E_INVALID; }
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// room for `points` stored points of which the first `keep` survive.  The capacity doubles; the new block is allocated beside the old one
// and filled by a device-to-device copy before the old one goes, so a failure changes nothing (peak: old + new block, at most three times
// the points stored)
int grow_store(dcreg_ctx *c, int64_t points, int64_t keep) {
    DevBuf<float> &b = c->kf.xyz;
    const size_t need = 3 * (size_t)points;
    if (b.holds(need)) return DCREG_OK;
    DevBuf<float> fresh;
    const size_t n = std::max<size_t>(std::max(need, 2 * b.cap()), 3);
    if (fresh.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        c->fail("hipMalloc(%zu B) failed while growing the keyframe store", n * sizeof(float));
        return DCREG_E_NOMEM;
    }
    if (b && keep) HIP_TRY(c, hipMemcpyAsync(fresh.data(), b.data(), 3 * (size_t)keep * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b.swap(fresh);
    return DCREG_OK;
}

// n packed points at `in` become the clouds off[0 .. n_clouds] behind the store's last keyframe; they count only when everything went well
int store_append(dcreg_ctx *c, const float4 *in, int n_clouds, const int64_t *off, int64_t *first_id) {
    dcreg_ctx::KeyframeBufs &B = c->kf;
    const int64_t n = n_clouds > 0 ? off[n_clouds] : 0, stored = B.off.back();
    if (stored + n > kKfMaxStored) { c->fail("the keyframe store would hold 2^32 or more points"); return DCREG_E_INVALID; }
    try { B.off.reserve(B.off.size() + (size_t)n_clouds); } catch (const std::bad_alloc &) { c->fail("out of host memory"); return DCREG_E_NOMEM; }
    uint32_t flag = 0;
    if (n > 0) {
        if (B.flag.ensure(c, 1)) return DCREG_E_NOMEM;
        if (int rc = grow_store(c, stored + n, stored)) return rc;
        HIP_TRY(c, hipMemsetAsync(B.flag.data(), 0, sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(k_kf_store, dim3(blocks(n, kKfBlock)), dim3(kKfBlock), 0, c->stream, in, n, B.xyz.data() + 3 * (size_t)stored, B.flag.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&flag, B.flag.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (flag) { c->fail("a keyframe cloud has non-finite coordinates"); return DCREG_E_INVALID; }
    if (first_id) *first_id = (int64_t)B.off.size() - 1;
    for (int s = 0; s < n_clouds; ++s) B.off.push_back(stored + off[s + 1]);
    return DCREG_OK;
}

int add_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, int64_t *first_id) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    if (int rc = check_clouds(c, n_clouds, xyz, off, stride)) return rc;
    const int64_t n = n_clouds > 0 ? off[n_clouds] : 0;
    if (n > 0)
        if (int rc = upload_cloud(c, xyz, n, stride, on_device, c->vox.pts)) return rc;
    return store_append(c, c->vox.pts.data(), n_clouds, off, first_id);
}

// The members of a call checked (every refusal of include/dcreg.h before anything is queued) and turned into the gather's records and the
// submaps' point offsets sub_off[n_submaps + 1]
int gather_prepare(dcreg_ctx *c, int64_t n_submaps, const int64_t *moff, const int64_t *ids, const double *poses, GatherRun &g,
                   std::vector<int64_t> &sub_off) {
    const dcreg_ctx::KeyframeBufs &B = c->kf;
    if (n_submaps < 0 || n_submaps >= INT32_MAX || (n_submaps > 0 && !moff)) { c->fail("invalid submap arguments"); return DCREG_E_INVALID; }
    if (n_submaps > 0 && moff[0] != 0) { c->fail("member offsets must start at 0"); return DCREG_E_INVALID; }
    for (int64_t s = 0; s < n_submaps; ++s)
        if (moff[s + 1] < moff[s]) { c->fail("member offsets decrease at submap %lld", (long long)s); return DCREG_E_INVALID; }
    const int64_t M = n_submaps > 0 ? moff[n_submaps] : 0, count = (int64_t)B.off.size() - 1;
    if (M > 0 && (!ids || !poses)) { c->fail("null member ids or poses"); return DCREG_E_INVALID; }
    g = GatherRun();
    try {
        sub_off.assign((size_t)n_submaps + 1, 0);
        int64_t n = 0;
        for (int64_t s = 0; s < n_submaps; ++s) {
            for (int64_t m = moff[s]; m < moff[s + 1]; ++m) {
                const int64_t id = ids[m];
                if (id < 0 || id >= count) {
                    c->fail("member %lld names keyframe %lld, the store holds [0, %lld)", (long long)m, (long long)id, (long long)count);
                    return DCREG_E_INVALID;
                }
                const double *P = poses + 12 * m;
                for (int e = 0; e < 12; ++e)
                    if (!std::isfinite(P[e])) { c->fail("the pose of member %lld has non-finite entries", (long long)m); return DCREG_E_INVALID; }
                const int64_t np = B.off[(size_t)id + 1] - B.off[(size_t)id];
                if (np == 0) continue;
                if (n + np >= kKfMaxCall) { c->fail("the members of one call hold 2^31 - 1 or more points"); return DCREG_E_INVALID; }
                if (g.members.size() >= (size_t)INT32_MAX - 1) { c->fail("too many members in one call"); return DCREG_E_INVALID; }
                KfMember r;
                r.start = (uint32_t)n;
                r.src = (uint32_t)B.off[(size_t)id];
                std::memcpy(r.pose, P, sizeof(r.pose));
                g.members.push_back(r);
                n += np;
            }
            sub_off[(size_t)s + 1] = n;
        }
        g.n = n;
    } catch (const std::bad_alloc &) {
        c->fail("out of host memory");
        return DCREG_E_NOMEM;
    }
    return DCREG_OK;
}

void raw_info(dcreg_voxel_info *info, int64_t n) {
    if (info) { info->n_in = info->n_finite = info->n_out = n; info->n_voxels = 0; }
}

// dcreg_keyframes_submaps*: raw - the gather writes 3 floats per point (straight into the caller's device memory, or into the context's
// buffer and from there to the host in one copy); with a voxel block - the gather packs for the voxel pass, whose output is copied out
int submaps(dcreg_ctx *c, int n_submaps, const int64_t *moff, const int64_t *ids, const double *poses, const dcreg_voxel_params *vp, float *out,
            int64_t capacity, int64_t *out_off, dcreg_voxel_info *info, bool out_on_device) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    if (!out_off || capacity < 0) { c->fail("invalid output arguments"); return DCREG_E_INVALID; }
    GatherRun g;
    std::vector<int64_t> sub_off;
    if (int rc = gather_prepare(c, n_submaps, moff, ids, poses, g, sub_off)) return rc;
    int64_t n_out = g.n;
    const float *from = nullptr;
    if (vp) {
        VoxelResult r;
        if (int rc = voxel_pass(c, n_submaps, nullptr, sub_off.data(), 3, true, vp, false, r, nullptr, &g)) return rc;
        out_off[0] = 0;
        for (int s = 0; s < n_submaps; ++s) out_off[s + 1] = out_off[s] + r.kept[(size_t)s];
        if (info) { info->n_in = r.n_in; info->n_finite = r.n_finite; info->n_voxels = r.n_voxels; info->n_out = r.n_out; }
        n_out = r.n_out;
        from = c->vox.out.data();
    } else {
        for (int s = 0; s <= n_submaps; ++s) out_off[s] = sub_off[(size_t)s];
        raw_info(info, g.n);
    }
    if (n_out > capacity) { c->fail("the output holds %lld points, the capacity is %lld", (long long)n_out, (long long)capacity); return DCREG_E_INVALID; }
    if (n_out > 0 && !out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    const size_t bytes = sizeof(float) * 3 * (size_t)n_out;
    if (n_out > 0 && !vp) {
        if (out_on_device) {
            if (int rc = gather_queue(c, g, nullptr, out)) return rc;
        } else {
            if (c->kf.out.ensure(c, 3 * (size_t)n_out)) return DCREG_E_NOMEM;
            if (int rc = gather_queue(c, g, nullptr, c->kf.out.data())) return rc;
            from = c->kf.out.data();
        }
    }
    if (n_out > 0 && from) if (int rc = caller_out(c, out, from, bytes, out_on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

}  // namespace

// the call's member records uploaded in one copy, then k_kf_gather over the g.n output points (g outlives the stream's work: every caller
// waits for the stream before it returns)
int gather_queue(dcreg_ctx *c, const GatherRun &g, float4 *out4, float *out3) {
    if (g.n <= 0) return DCREG_OK;
    dcreg_ctx::KeyframeBufs &B = c->kf;
    const size_t nm = g.members.size();
    if (B.members.ensure(c, nm)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemcpyAsync(B.members.data(), g.members.data(), sizeof(KfMember) * nm, hipMemcpyHostToDevice, c->stream));
    const dim3 grid(blocks(g.n, kKfTile)), block(kKfBlock);
    if (out3) {
        const int vec3 = (reinterpret_cast<uintptr_t>(out3) & 15u) == 0u ? 1 : 0;
        hipLaunchKernelGGL(k_kf_gather<true>, grid, block, 0, c->stream, B.xyz.data(), B.members.data(), (int)nm, g.n, (float4 *)nullptr, out3, vec3);
    } else {
        hipLaunchKernelGGL(k_kf_gather<false>, grid, block, 0, c->stream, B.xyz.data(), B.members.data(), (int)nm, g.n, out4, (float *)nullptr, 0);
    }
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

}  // namespace dcreg

using namespace dcreg;

static_assert(sizeof(KfMember) == 104, "one member record is 104 B (include/dcreg.h states it)");

extern "C" {

int dcreg_keyframes_reset(dcreg_ctx *c) {
    if (int rc = enter(c)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->kf.xyz.reset();
    c->kf.off.assign(1, 0);
    c->kf.ready = true;
    return DCREG_OK;
}

int64_t dcreg_keyframes_count(const dcreg_ctx *c) { return c && c->kf.ready ? (int64_t)c->kf.off.size() - 1 : 0; }

int dcreg_keyframes_sizes(const dcreg_ctx *cc, int64_t first, int64_t n, int64_t *n_points) {
    dcreg_ctx *c = const_cast<dcreg_ctx *>(cc);
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    const int64_t count = (int64_t)c->kf.off.size() - 1;
    if (first < 0 || n < 0 || first > count || n > count - first) {
        c->fail("the range [%lld, %lld + %lld) is not inside the store's [0, %lld)", (long long)first, (long long)first, (long long)n, (long long)count);
        return DCREG_E_INVALID;
    }
    if (n > 0 && !n_points) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    for (int64_t k = 0; k < n; ++k) n_points[k] = c->kf.off[(size_t)(first + k) + 1] - c->kf.off[(size_t)(first + k)];
    return DCREG_OK;
}

int dcreg_keyframes_add_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, int64_t *first_id) {
    return add_clouds(c, n_clouds, xyz, offsets, stride_floats, false, first_id);
}
int dcreg_keyframes_add_clouds_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats, int64_t *first_id) {
    return add_clouds(c, n_clouds, d_xyz, offsets, stride_floats, true, first_id);
}

int dcreg_keyframes_add_source(dcreg_ctx *c, int64_t *id) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    const int64_t off[2] = {0, c->n_src};
    return store_append(c, c->d_src_raw.data(), 1, off, id);
}

int dcreg_keyframes_get(dcreg_ctx *c, int64_t id, float *xyz_out, int64_t capacity_points) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    const int64_t count = (int64_t)c->kf.off.size() - 1;
    if (id < 0 || id >= count) { c->fail("keyframe %lld is not inside the store's [0, %lld)", (long long)id, (long long)count); return DCREG_E_INVALID; }
    const int64_t b = c->kf.off[(size_t)id], n = c->kf.off[(size_t)id + 1] - b;
    if (capacity_points < n || (n > 0 && !xyz_out)) {
        c->fail("the output holds %lld points, the keyframe %lld", (long long)capacity_points, (long long)n);
        return DCREG_E_INVALID;
    }
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(xyz_out, c->kf.xyz.data() + 3 * (size_t)b, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

int dcreg_keyframes_submaps(dcreg_ctx *c, int n_submaps, const int64_t *member_offsets, const int64_t *member_ids, const double *member_poses,
                            const dcreg_voxel_params *voxel, float *out_xyz, int64_t capacity_points, int64_t *out_offsets, dcreg_voxel_info *vinfo) {
    return submaps(c, n_submaps, member_offsets, member_ids, member_poses, voxel, out_xyz, capacity_points, out_offsets, vinfo, false);
}
int dcreg_keyframes_submaps_device(dcreg_ctx *c, int n_submaps, const int64_t *member_offsets, const int64_t *member_ids, const double *member_poses,
                                   const dcreg_voxel_params *voxel, float *d_out_xyz, int64_t capacity_points, int64_t *out_offsets,
                                   dcreg_voxel_info *vinfo) {
    return submaps(c, n_submaps, member_offsets, member_ids, member_poses, voxel, d_out_xyz, capacity_points, out_offsets, vinfo, true);
}

int dcreg_set_target_keyframes(dcreg_ctx *c, int64_t n_members, const int64_t *member_ids, const double *member_poses,
                               const dcreg_voxel_params *voxel, double search_radius_hint, dcreg_voxel_info *vinfo) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    if (n_members <= 0) { c->fail("a target needs at least one member"); return DCREG_E_INVALID; }
    const int64_t moff[2] = {0, n_members};
    GatherRun g;
    std::vector<int64_t> sub_off;
    if (int rc = gather_prepare(c, 1, moff, member_ids, member_poses, g, sub_off)) return rc;
    return set_target_gathered(c, g, voxel, search_radius_hint, vinfo);
}

}  // extern "C"
