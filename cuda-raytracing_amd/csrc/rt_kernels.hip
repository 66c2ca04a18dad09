// rt_kernels.hip -- the raycast hot path for MI355X (gfx950, wave64) and its C-ABI (include/rt_hip.h).
//
// Path replaced: render<<<>>> / cast_ray (raycast.cu:146-297 / :21-142) with everything they
// call (d_BVHTree::ray_intersects BVHTree.hpp:40-54, TrianglePrimitive::ray_intersect /
// point_inside TrianglePrimitive.hpp:62-79,151-185, the L0 math in utils.hpp / transforms.hpp).
// Results are bit-identical to the reference arithmetic (see rt_math.h); the memory layout and
// the execution mapping are not the reference's -- see DESIGN.md.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (mandatory: SURVEY.md H3) -fno-slp-vectorize (see _build.py).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_device_types.h"
#include "rt_math.h"
#include "rt_scene_internal.h"

using namespace rt;

// The traversal code below holds ONE form of everything: the forms that were measured against it and lost (the round-5 text of the
// hand-written loop, a wave-level stack check, Z-order lanes, flag forms of the sentinel loop, the bounce kernel's secondary rays through
// the hand-written loop, ...) live in history; their logs under profiles/r0*_experiments/ name the commits that hold them.  An A/B
// experiment is a variant library built with RT_HIPCC_EXTRA (tools/build_variant.sh), not a switch kept here.

// =====================================================================================
//                                      device code
// =====================================================================================

namespace {

constexpr int kBlock = 256;     // the extension kernels' workgroup: one 16x16-pixel tile = 2x2 wave tiles of 8x8 pixels
constexpr int kTile = 16;
// The primary kernels' workgroup is ONE wave = one 8x8-pixel tile (round 5).  A 256-thread workgroup keeps its LDS block until its
// last wave has finished, and no new workgroup fits a CU whose LDS is taken by eight of them: the slots of waves that finished
// early stood empty -- SQ_WAVE_CYCLES put the average residency at 6.7 of 8 waves per SIMD.  With one wave per workgroup a slot is
// refilled the moment its wave ends: c2 far / mid / near -7.7 % / -3.4 % / -4.2 % (profiles/r05_experiments/asm_loop_ab.log).
// (Round 2 measured this form at +-2 %: the kernel of that round was bound by its instruction count, not by waves waiting.)
constexpr int kPrimBlock = 64;
constexpr int kPrimTile = 8;

struct Hit {
    float min;                  // HitInfo::min, raycast.cu:12
    int32_t slot;               // triangle slot of the accepted hit
    int32_t instance;
    float u, v;                 // barycentrics of the accepted hit (uv is interpolated once, at shade time) -- or, for a mesh in the
                                // exact-uv mode, the interpolated uv itself (the two never coexist: two registers, not four)
    V3 loc;                     // world-space location of the accepted hit (extension kernel only)
};

// d_BVHTree::ray_intersects, BVHTree.hpp:40-54, from the six differences (box min - origin, box max - origin):
// the subtraction is done where the record is fetched, see trace_instance.
__device__ __forceinline__ float slab(float dnx, float dny, float dnz, float dxx, float dxy, float dxz, V3 dinv)
{
    float tminx = dnx * dinv.x, tminy = dny * dinv.y, tminz = dnz * dinv.z;
    float tmaxx = dxx * dinv.x, tmaxy = dxy * dinv.y, tmaxz = dxz * dinv.z;
    float t1x = fminf(tminx, tmaxx), t1y = fminf(tminy, tmaxy), t1z = fminf(tminz, tmaxz);
    float t2x = fmaxf(tminx, tmaxx), t2y = fmaxf(tminy, tmaxy), t2z = fmaxf(tminz, tmaxz);
    float dst_far = fminf(fminf(t2x, t2y), t2z);
    float dst_near = fmaxf(fmaxf(t1x, t1y), t1z);
    bool hit = dst_far >= dst_near && dst_far > 0.0f;
    return hit ? dst_near : FLT_MAX;
}

// The same test for a ray whose sign octant is known at compile time (OCT bit k set = dinv component k negative): with
// box.min <= box.max, a finite origin and a finite non-zero dinv, rounding is monotone, so fl((min-o)*dinv) <= fl((max-o)*dinv)
// for dinv > 0 and the reverse for dinv < 0 -- which of the two products is the near one and which the far one is a choice
// of operand per axis, not an instruction.  The values equal fminf / fmaxf of the pair except for the sign of a zero, which
// no compare below can see.  (12 VALU fewer per interior node; trace_instance checks the preconditions per wave.)
template <int OCT>
__device__ __forceinline__ float slab_oct(float dnx, float dny, float dnz, float dxx, float dxy, float dxz, V3 dinv)
{
    float t1x = ((OCT & 1) ? dxx : dnx) * dinv.x, t2x = ((OCT & 1) ? dnx : dxx) * dinv.x;
    float t1y = ((OCT & 2) ? dxy : dny) * dinv.y, t2y = ((OCT & 2) ? dny : dxy) * dinv.y;
    float t1z = ((OCT & 4) ? dxz : dnz) * dinv.z, t2z = ((OCT & 4) ? dnz : dxz) * dinv.z;
    float dst_far = fminf(fminf(t2x, t2y), t2z);
    float dst_near = fmaxf(fmaxf(t1x, t1y), t1z);
    bool hit = dst_far >= dst_near && dst_far > 0.0f;
    return hit ? dst_near : FLT_MAX;
}

// The first twelve words of an interior record are the two child boxes (min xyz, max xyz each); this turns them into
// box - origin, written over the record's registers q0..q2.  W = the record itself, or the 16-word scalar-register
// vector of a wave-uniform fetch: the subtraction then takes its box operand from the scalar register directly and the
// record never has to be copied into vector registers.
template <class W>
__device__ __forceinline__ void box_differences(const W& w, V3 o, float4& q0, float4& q1, float4& q2)
{
    q0 = make_float4(w[0] - o.x, w[1] - o.y, w[2] - o.z, w[3] - o.x);
    q1 = make_float4(w[4] - o.y, w[5] - o.z, w[6] - o.x, w[7] - o.y);
    q2 = make_float4(w[8] - o.z, w[9] - o.x, w[10] - o.y, w[11] - o.z);
}

// Primary ray direction of pixel (x, y), raycast.cu:159-188, in two halves that every caller runs back to back.
// camera_space_direction: raycast.cu:159-182, the part that depends on (K_inv, D, x, y) only -- the same in every frame of a launch
// whose frames share their intrinsics, which is what the direction table holds (RenderParams::dir_table).
__device__ __forceinline__ V3 camera_space_direction(const FrameParams& p, float fx, float fy)
{
    // apply_matrix(K_inv, (x, y, 1)), utils.hpp:134-140
    float a = p.kinv[0] * fx + p.kinv[1] * fy + p.kinv[2] * 1.0f;
    float b = p.kinv[3] * fx + p.kinv[4] * fy + p.kinv[5] * 1.0f;
    float c = p.kinv[6] * fx + p.kinv[7] * fy + p.kinv[8] * 1.0f;
    float radius = sqrtf(a * a + b * b);
    float theta = atanf_fdlibm(radius);
    // raycast.cu:172 -- float products, double sum, double outer product, narrowed to float
    float thetad = (float)((double)theta * (1.0 + (double)(p.D[0] * theta) + (double)(p.D[1] * theta * theta)
                   + (double)(p.D[2] * theta * theta * theta) + (double)(p.D[3] * theta * theta * theta * theta)));
    float scale = thetad / radius;
    V3 d = normalize(v3(scale * a, scale * b, c));
    return v3(d.x, d.z, -d.y);                                  // raycast.cu:182
}

// ... and the frame's part: the camera's rotation and the final normalize
__device__ __forceinline__ V3 world_direction(const FrameParams& p, V3 d)
{
    d = apply_quat(p.q_cam, d);                                 // raycast.cu:185
    return normalize(d);                                        // raycast.cu:188
}

template <bool DEBUG>
struct Counters {
    int pops = 0, aabb = 0, tris = 0, inside = 0;
};
template <>
struct Counters<false> {};

// Per-lane traversal stack (raycast.cu:54-61).  The first `lds_depth` entries live in LDS, one column per lane
// ([entry][kBlock] ints: a wave's accesses are conflict-free); deeper entries -- rare: the tree may be 28+ levels
// deep but rays seldom hold more than a dozen postponed nodes -- spill to a private (scratch) array.  Keeping the
// LDS part at 16 entries (+ the sentinel's row) lets 8 waves/SIMD stay resident (17 KB per 256-thread workgroup, 136 of 160 KB).
constexpr int kLdsStack = 16;
// Two entries no tree contains: leaf references whose slot field is beyond every slot a scene can hold (rt_scene_upload and the
// rebuild keep slot_base + n + 1 <= kSlotMask, so the largest first-slot of a leaf is kSlotMask - 2).  Chosen among the
// hardware's inline integer constants (-16 .. 64): compares and selects against them need no register.
// kSentinel: the first entry of every traversal; popping it ends the loop.
// kNeedPop: what interior_apply / the leaf step leave in `cur` when the lane has to pop.
constexpr int32_t kSentinel = -2;               // = leaf flag | count 31 | slot kSlotMask - 1
constexpr int32_t kNeedPop = -1;                // = leaf flag | count 31 | slot kSlotMask
static_assert((kSentinel & kSlotMask) == kSlotMask - 1 && (kNeedPop & kSlotMask) == kSlotMask, "beyond the slot space");
// rows of a workgroup's LDS stack block ([row][thread] ints): the postponed nodes kept in LDS, plus the sentinel's row
__host__ __device__ inline int lds_rows(int stack_depth) { return (stack_depth < kLdsStack ? stack_depth : kLdsStack) + 1; }
typedef __attribute__((address_space(3))) int lds_int;      // typed LDS pointer: keeps stack traffic on ds_read/ds_write
// SPILL = false: the tree is shallow enough for the LDS part alone (a tree of L levels never holds more than L - 1 postponed
// nodes: the entries of a stack sit at strictly increasing levels below the root) -- no private array, and neither push
// nor pop carries the "which memory" branch (5 + 4 scalar instructions of exec-mask bookkeeping per iteration).
// OPTIMISTIC (with SPILL = false, for trees that ARE deeper than the LDS part): the block has one more row, which takes the
// push that does not fit; interior_apply then hands the lane the sentinel, the lane leaves its loop with sp != 0, and the
// caller traces that ray again from the start on a SPILL stack.  Which rays need more than 16 postponed nodes depends on the
// view (none of the three c2 cameras has one in a 28-level tree), so the common case pays two vector instructions per push
// instead of nine scalar ones per iteration.
template <int STRIDE, bool SPILL = true, bool OPTIMISTIC = false>   // STRIDE = threads per workgroup (ints between two entries of a lane)
struct StackT {
    static constexpr bool kOptimistic = OPTIMISTIC;
    static constexpr bool kSpill = SPILL;
    static constexpr int kStride = STRIDE;
    static_assert(!(SPILL && OPTIMISTIC), "the optimistic stack is the LDS-only one");
    lds_int* lds;               // this lane's LDS column
    int* spill;                 // this lane's private overflow, kMaxStack - kLdsStack entries
    int lds_depth;              // entries kept in LDS: lds_rows(stack_depth)
    int sp;
    // (Asking once per wave whether ANY lane is beyond the LDS part costs what the per-lane "which memory" regions cost: measured
    // +0.8 % on c2, profiles/r04_experiments/sentinel_loop_ab.log.)
    __device__ __forceinline__ void push(int32_t v)
    {
        if constexpr (SPILL) { if (sp < lds_depth) lds[sp * STRIDE] = v; else spill[sp - lds_depth] = v; }
        else lds[sp * STRIDE] = v;
        sp++;
    }
    __device__ __forceinline__ int32_t pop()
    {
        --sp;
        if constexpr (!SPILL) return lds[sp * STRIDE];
        // always an LDS read (index clamped) and, rarely, a private read on top: a select between the two
        // address spaces would turn into one slow flat_load
        int32_t v = lds[(sp < lds_depth ? sp : lds_depth - 1) * STRIDE];
        if (sp >= lds_depth) v = spill[sp - lds_depth];
        return v;
    }
};

typedef StackT<kBlock> Stack;

// Ray in mesh space (raycast.cu:33-51) plus what the leaf code needs of the instance.
struct MeshRay {
    V3 ro, rd, dinv;
};

__device__ __forceinline__ MeshRay to_mesh_space(const DevInstance& in, V3 org, V3 dir)
{
    MeshRay r;
    r.rd = apply_quat(in.q_rot, dir);
    r.rd.x *= in.inv_scale[0]; r.rd.y *= in.inv_scale[1]; r.rd.z *= in.inv_scale[2];
    r.ro = apply_quat(in.q_pose, v3(org.x - in.pose_xyz[0], org.y - in.pose_xyz[1], org.z - in.pose_xyz[2]));
    r.ro.x *= in.inv_scale[0]; r.ro.y *= in.inv_scale[1]; r.ro.z *= in.inv_scale[2];
    r.dinv = v3(1.0f / r.rd.x, 1.0f / r.rd.y, 1.0f / r.rd.z);  // Ray.hpp:21
    return r;
}

// The ray header of (frame, instance) (RayHeader; view_records_kernel writes it): one fetch through the scalar cache, the words
// staying in scalar registers.  `view_off` = byte offset of the frame's view from p.records.
struct RayHeaderWords {
    V3 ro; uint32_t flags; Q4 q_rot; V3 inv_scale; int32_t root_ref; V3 back; uint32_t vdelta;
};
static_assert(offsetof(RayHeader, flags) == 12 && offsetof(RayHeader, q_rot) == 16 && offsetof(RayHeader, inv_scale) == 32 &&
              offsetof(RayHeader, root_ref) == 44 && offsetof(RayHeader, inv_pose_xyz) == 48 && offsetof(RayHeader, vdelta) == 60, "RayHeader layout");

__device__ __forceinline__ RayHeaderWords ray_header(const RenderParams& p, uint32_t view_off, int inst_index)
{
    // (four quarters, not one sixteen-register value: the allocator keeps or drops a fetched value whole, and only the last quarter
    // lives on into the loop)
    typedef float f4v __attribute__((ext_vector_type(4)));
    f4v w0, w1, w2, w3;
    const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)(view_off + (uint32_t)inst_index * (uint32_t)sizeof(RayHeader)));
    asm volatile("s_load_dwordx4 %0, %4, %5\n\ts_load_dwordx4 %1, %4, %5 offset:16\n\ts_load_dwordx4 %2, %4, %5 offset:32\n\t"
                 "s_load_dwordx4 %3, %4, %5 offset:48\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(w0), "=&s"(w1), "=&s"(w2), "=&s"(w3) : "s"(p.records), "s"(off));
    RayHeaderWords h;
    h.ro = v3(w0[0], w0[1], w0[2]); h.flags = __float_as_uint(w0[3]);
    h.q_rot.x = w1[0]; h.q_rot.y = w1[1]; h.q_rot.z = w1[2]; h.q_rot.w = w1[3];
    h.inv_scale = v3(w2[0], w2[1], w2[2]); h.root_ref = __float_as_int(w2[3]);
    h.back = v3(w3[0], w3[1], w3[2]); h.vdelta = __float_as_uint(w3[3]);
    return h;
}

// (the direction's half of to_mesh_space above, operation for operation; the origin is the header's)
__device__ __forceinline__ MeshRay to_mesh_space(const RayHeaderWords& h, V3 dir)
{
    MeshRay r;
    r.rd = apply_quat(h.q_rot, dir);
    r.rd.x *= h.inv_scale.x; r.rd.y *= h.inv_scale.y; r.rd.z *= h.inv_scale.z;
    r.ro = h.ro;
    r.dinv = v3(1.0f / r.rd.x, 1.0f / r.rd.y, 1.0f / r.rd.z);
    return r;
}

// One interior node (raycast.cu:66-79) from its already fetched 64-B record: tests both children, pushes the
// far one if it passes `dist < hit.min`, and leaves in `cur` the entry the reference would pop next (the entry
// pushed last never goes through the stack).  Returns false when nothing was pushed.
// W: the record's first fourteen words, box words already as box - origin: an array of the lane's registers, or the scalar-register
// vector of a wave-uniform fetch of a VIEW record (the products of the slab test then take their box operand from the scalar
// register: no copy, no subtraction).
template <bool DEBUG, class STK, int OCT = -1, bool NEED_POP = false, class W>
__device__ __forceinline__ bool interior_apply_words(const W& w, const MeshRay& r, float hit_min,
                                                     int32_t& cur, STK& stack, Counters<DEBUG>& cnt)
{
    int32_t ra = __float_as_int(w[12]), rb = __float_as_int(w[13]);
    if constexpr (DEBUG) cnt.aabb += 2;
    float da, db;                                                       // w[0..11]: box - origin (box_differences, or a view record)
    if constexpr (OCT < 0) {
        da = slab(w[0], w[1], w[2], w[3], w[4], w[5], r.dinv);
        db = slab(w[6], w[7], w[8], w[9], w[10], w[11], r.dinv);
    } else {
        da = slab_oct<OCT>(w[0], w[1], w[2], w[3], w[4], w[5], r.dinv);
        db = slab_oct<OCT>(w[6], w[7], w[8], w[9], w[10], w[11], r.dinv);
    }
    // push order of raycast.cu:72-79: the farther child is pushed first, the nearer one last (= popped next); each only if
    // its distance passes `dist < hit.min`.  With pa / pb = "child a / b passes": both pass -> push the far one (b when
    // da < db, else a -- a tie takes the else branch) and go on with the near one; one passes -> go on with that one (it is
    // the nearer: the other failed the same bound); none -> the caller pops.  (da, db are never NaN: slab returns a
    // distance or FLT_MAX; a NaN hit_min fails every compare, as in the reference.)
    const bool a_near = da < db;
    const bool pa = da < hit_min, pb = db < hit_min;
    int32_t next = pa ? ra : rb;
    if (pa && pb) {
        stack.push(a_near ? rb : ra);                           // the only entry that really goes through the stack
        next = a_near ? ra : rb;
        // (optimistic stack: that push went to the spare row -- this lane is done here and will be traced again, see StackT)
        if constexpr (STK::kOptimistic) next = stack.sp > stack.lds_depth ? kSentinel : next;
    }
    cur = NEED_POP ? ((pa | pb) ? next : kNeedPop) : next;      // (without NEED_POP: not used when neither passed, the caller pops)
    return pa || pb;
}

template <bool DEBUG, class STK, int OCT = -1, bool NEED_POP = false>
__device__ __forceinline__ bool interior_apply(float4 q0, float4 q1, float4 q2, float4 q3, const MeshRay& r, float hit_min,
                                               int32_t& cur, STK& stack, Counters<DEBUG>& cnt)
{
    const float w[14] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y};
    return interior_apply_words<DEBUG, STK, OCT, NEED_POP>(w, r, hit_min, cur, stack, cnt);
}

// What a triangle test proposes as the new closest hit.  Deliberately left uninitialised by the callers: it is only
// read where triangle_test returned true.
struct Candidate {
    float dist, u, v;
    float2 uv;
    V3 loc;
};

// One triangle of a leaf (one iteration of raycast.cu:85-136) from its already fetched 64-B record t0..t3.
// Returns whether the reference would accept it as the new closest hit (raycast.cu:109) and fills `c` in that case;
// the caller applies the update with selects at the top level of its loop, which keeps the hit record out of the
// control flow (as branch-merged values it cost two register copies per field per loop iteration).
template <bool DEBUG, bool EX>
__device__ __forceinline__ bool triangle_test(const RenderParams& p, const DevInstance& in, bool exact_uv, bool identity_inv,
                                              const MeshRay& r, V3 org, int slot, float hit_min, Counters<DEBUG>& cnt,
                                              float4 t0, float4 t1, float4 t2, float4 t3, Candidate& c)
{
    if constexpr (DEBUG) cnt.tris++;
    V3 v0 = v3(t0.x, t0.y, t0.z), nrm = v3(t0.w, t1.x, t1.y);
    // The reference's chain of early returns (TrianglePrimitive.hpp:66,72, raycast.cu:91,96) is evaluated as
    // one predicate over straight-line code: a wave almost always has some lane that passes each test, so
    // branching per test only adds exec-mask bookkeeping.  Lanes whose predicate is already false compute
    // on garbage that is never used.
    // TrianglePrimitive::ray_intersect, TrianglePrimitive.hpp:62-79
    float denom = dot(r.rd, nrm);
    // `abs(denom) < 1e-6` compares in double; 0x358637be is the smallest float whose double value is >= 1e-6,
    // so this float compare selects exactly the same floats (tests/test_host_logic.py checks the boundary).
    bool ok = !(fabsf(denom) < __int_as_float(0x358637be));
    // A candidate is only ever accepted when same_dir = denom < 0 (raycast.cu:107-109); for denom >= 0 (or NaN)
    // the rest of the test has no observable effect, so the production kernel drops it here.  The debug kernel
    // goes on because the inside-hit count of raycast.cu:96 is one of the parity planes.
    if constexpr (!DEBUG) ok = ok && (denom < 0.0f);
    float tt = dot(v0 - r.ro, nrm) / denom;
    ok = ok && !(tt < 0.0f);
    V3 pt = r.ro + tt * r.rd;
    ok = ok && !(pt.x == FLT_MAX);                          // raycast.cu:91
    // TrianglePrimitive::point_inside, TrianglePrimitive.hpp:151-185
    V3 e0 = v3(t1.z, t1.w, t2.x), e1 = v3(t2.y, t2.z, t2.w);
    V3 e2 = pt - v0;
    float dot02 = dot(e0, e2), dot12 = dot(e1, e2);
    float u = (t3.z * dot02 - t3.y * dot12) * t3.w;
    float v = (t3.x * dot12 - t3.y * dot02) * t3.w;
    ok = ok && (u >= 0.0f) && (v >= 0.0f) && (u + v <= 1.0f);
    c.u = u; c.v = v;
    if (exact_uv) {
        c.uv = make_float2(0.0f, 0.0f);
        if (ok) {                                           // raycast.cu:96 can only fail for absurd uv data
            const float* q = p.tri_uv + (size_t)slot * 6;
            float w = 1.0f - u - v;
            c.uv.x = (w * q[0] + v * q[2]) + u * q[4];
            c.uv.y = (w * q[1] + v * q[3]) + u * q[5];
            ok = c.uv.x != FLT_MAX;
        }
    }
    bool accept = false;
    if (ok) {
        if constexpr (DEBUG) cnt.inside++;
        // raycast.cu:98-104.  For an instance whose mesh -> world transform is exactly the identity (scale 1,
        // translation 0, quaternion (1,0,0,0): the common case) the scale / translate / rotate sequence returns
        // pt itself up to the sign of zero components, which the squares in magnitude() cannot see -- so the
        // production kernel skips it.  (The extension kernel keeps it: it stores `loc`.)
        V3 loc = pt;
        if (EX || !identity_inv) {
            loc = v3(pt.x * in.scale[0], pt.y * in.scale[1], pt.z * in.scale[2]);
            loc = apply_quat(in.q_inv_pose, v3(loc.x - in.inv_pose_xyz[0], loc.y - in.inv_pose_xyz[1], loc.z - in.inv_pose_xyz[2]));
        }
        c.dist = magnitude(loc - org);
        if constexpr (EX) c.loc = loc;
        // raycast.cu:107-109: same_dir = dot(r_ray.direction, normal) is `denom`
        // (bitwise: as `&&` / `||` the compiler builds a chain of exec-mask regions for the three compares)
        accept = (denom < 0) & ((hit_min == FLT_MAX) | (c.dist < hit_min));
    }
    return accept;
}

// The workgroup's linear index in its grid -- (tiles_x, tiles_y, frames) for un-ordered primary launches: frame-major, then tile
// rows -- which is the row of RenderParams::trace its waves write (render_kernel's stamps, trace_loop<.., PROF>'s phase sums).
__device__ __forceinline__ size_t trace_workgroup() { return ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// One instance of raycast.cu:26-139.
//
// Interior nodes and triangles are both 64-B records of ONE array, so every lane issues the same four 16-B loads at
// `records + (entry << 6)` ("unified fetch") and the wave waits for memory once per iteration, whatever mix of
// interior and leaf entries its lanes hold.  Each lane still visits exactly the reference's sequence of nodes.
// PROF = diagnostic copy with s_memtime stamps per phase (RT_TRACE_FILE); its frames are never timed.
// COUNT: *iters counts this lane's loop iterations (the cost measure behind the heavy-first dispatch order).
// POPS (the extension kernel): *pops counts the lane's node pops, the one visit count that kernel reports.
// OCT >= 0: every lane of the wave is known to hold a ray of sign octant OCT that meets slab_oct's preconditions.
// ANYHIT (the extension's shadow rays, rt_occluded): raycast.cu:129-133 restored -- cast_ray(..., lighting_pass = true, light_distance =
// tmax) returns at the first accepted hit whose distance is below light_distance (FLT_MAX for shadow rays, per ray for rt_occluded).
// VIEW (primary rays of render_kernel<.., VIEW>): interior records are read from the frame's view records, `vdelta` bytes behind the
// record itself, whose box words already are box - r.ro (view_records_kernel: the same subtraction, done once per frame and
// instance instead of per visit and lane); an iteration in which the whole wave holds the same interior node takes them as
// scalar operands and skips the leaf half of the loop altogether.
template <bool DEBUG, bool PROF, bool EX, bool COUNT, class STK, bool POPS, int OCT, bool ANYHIT = false, bool VIEW = false>
__device__ __forceinline__ void trace_loop(const RenderParams& p, const DevInstance& in, int inst_index, const MeshRay& r,
                                           V3 org, STK& stack, Hit& hit, Counters<DEBUG>& cnt, int* iters, int* pops, uint32_t vdelta = 0,
                                           float tmax = FLT_MAX)
{
    static_assert(!VIEW || (!DEBUG && !PROF && !EX), "view records: the timed primary kernels only");
    stack.sp = 0;
    // The stack starts with a sentinel (raycast.cu:58 starts it with the root, which here stays in a register): "pop from an
    // empty stack" (raycast.cu:60) is then an ordinary pop that returns the sentinel, and the loop ends on the VALUE popped --
    // one compare for all lanes at the bottom of the loop instead of an `if (sp == 0) break` nested in the pop branch, which
    // cost ten scalar instructions of exec-mask bookkeeping per iteration.
    stack.push(kSentinel);
    int32_t cur = in.root_ref;                                  // raycast.cu:58 (kept in a register)
    bool have = true;
    // "this lane must pop" as a value of `cur` instead of the flag `have`: -1.5 % on the primary kernel, +0.8 % on the bounce
    // casts of the extension kernel (EX: they keep the flag) -- profiles/r04_experiments/sentinel_loop_ab.log
    constexpr bool kNeedPopValue = !EX;
    int rem = -1;                                               // triangles left in the leaf being walked, -1 = not in a leaf
    unsigned long long c_pop = 0, c_mem = 0, c_int = 0, c_leaf = 0, n_it = 0, n_int = 0, n_leaf = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    unsigned long long n_g1 = 0, n_g2 = 0, n_g34 = 0;
    // One iteration = one interior node or ONE triangle of a leaf (a leaf with k triangles takes k iterations and
    // keeps `cur` pointing at its next slot), so the loop has no inner loop and every record -- node or triangle,
    // first or later -- comes through the same fetch below.
    // The loop is bottom-tested (the pop and the stack-empty exit of raycast.cu:60-61 close the iteration) so that the
    // hit record leaves the loop after its update: with the exit at the top it was live across the back edge in two
    // copies.
    const bool exact_uv = in.exact_uv != 0, identity_inv = in.identity_inv != 0;    // (read once, not per triangle)
    do {
        if constexpr (PROF) t1 = __builtin_amdgcn_s_memtime();
        if constexpr (COUNT) (*iters)++;
        const bool interior = cur >= 0;
        if constexpr (DEBUG) cnt.pops += (interior || rem < 0) ? 1 : 0;
        if constexpr (POPS) *pops += (interior || rem < 0) ? 1 : 0;
        // About half of all wave iterations (three quarters for close-up views) find every active lane holding
        // the SAME entry -- coherent rays walk the top of the tree in lockstep.  Those iterations fetch the record
        // once per wave through the scalar cache (s_load_dwordx16) instead of 64 x 64 B through the vector memory
        // path, which is otherwise the busiest unit of the kernel (-9..-13 % frame time).
        float4 r0, r1, r2, r3;          // the record; for interior lanes r0..r2 become child boxes - ray origin
        const int32_t cur0 = __builtin_amdgcn_readfirstlane(cur);
        typedef float f16v __attribute__((ext_vector_type(16)));
        if constexpr (VIEW) {
            const bool one_entry = __ballot(cur != cur0) == 0ull;   // (wave-uniform) every lane holds the same entry
            if (one_entry && cur0 >= 0) {
                // The whole wave at one interior node: its VIEW record (box words = box - r.ro already) through the scalar cache,
                // used where it arrives -- as scalar operands of the slab products.  The iteration closes itself: no lane is at a leaf.
                f16v w;
                const uint32_t off = ((uint32_t)cur0 << 6) + vdelta;
                asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(p.records), "s"(off));
                have = interior_apply_words<DEBUG, STK, OCT, kNeedPopValue>(w, r, hit.min, cur, stack, cnt);
                if (kNeedPopValue ? cur == kNeedPop : !have) cur = stack.pop();
                __builtin_amdgcn_wave_barrier();
                continue;                                       // (to the bottom test: the sentinel may have been popped)
            }
            if (one_entry) {
                // the whole wave at one triangle record: copied for the code the per-lane fetch shares (through an OR with a zero
                // the optimiser cannot see through: plain copies are hoisted above the branch and run in every iteration)
                f16v w;
                const uint32_t off = (uint32_t)cur0 << 6;
                asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(p.records), "s"(off));
                int z;
                asm volatile("v_mov_b32 %0, 0" : "=v"(z));
                auto keep = [z](float f) { return __int_as_float(__float_as_int(f) | z); };
                r0 = make_float4(keep(w[0]), keep(w[1]), keep(w[2]), keep(w[3]));
                r1 = make_float4(keep(w[4]), keep(w[5]), keep(w[6]), keep(w[7]));
                r2 = make_float4(keep(w[8]), keep(w[9]), keep(w[10]), keep(w[11]));
                r3 = make_float4(keep(w[12]), keep(w[13]), keep(w[14]), keep(w[15]));
            } else {
                const uint32_t boff = ((uint32_t)cur << 6) + (interior ? vdelta : 0u);
                const float4* rec = (const float4*)((const char*)p.records + boff);
                r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
            }
        } else
        if (!PROF && __ballot(cur != cur0) == 0ull) {
            f16v w;
            // inline asm: hipcc would otherwise merge this load with the per-lane one below into a single vector load.
            // No "memory" clobber: the records are read-only, and a clobber makes every other load in the loop
            // (instance fields, ...) repeat each iteration.
            // The record's byte offset goes into the instruction's scalar offset operand (no 64-bit address arithmetic):
            // entry << 6 drops the flag and count bits of a leaf reference and stays below 4 GiB (at most 2^26 - 2 records).
            const uint32_t off = (uint32_t)cur0 << 6;
            asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(p.records), "s"(off));
            if (cur0 >= 0) {                                    // (a scalar branch: the whole wave holds this interior node)
                box_differences(w, r.ro, r0, r1, r2);
            } else {
                // (a triangle record is used as it is.  The copies go through an OR with a zero the optimiser cannot
                // see through: as plain copies they are hoisted above the branch and run for interior nodes too.)
                int z;
                asm volatile("v_mov_b32 %0, 0" : "=v"(z));
                auto keep = [z](float f) { return __int_as_float(__float_as_int(f) | z); };
                r0 = make_float4(keep(w[0]), keep(w[1]), keep(w[2]), keep(w[3]));
                r1 = make_float4(keep(w[4]), keep(w[5]), keep(w[6]), keep(w[7]));
                r2 = make_float4(keep(w[8]), keep(w[9]), keep(w[10]), keep(w[11]));
            }
            r3 = make_float4(w[12], w[13], w[14], w[15]);
        } else {
            const float4* rec = p.records + (size_t)(cur & kSlotMask) * 4;     // node or triangle: one array, one index space
            r0 = rec[0]; r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
            // (Every later use of r0..r3 gets its own s_waitcnt vmcnt(n), also on the path that issued no vector load.  Waiting for all
            // four loads HERE saves ten instructions per iteration and costs 0.5 % MORE time: the subtractions of box_differences no
            // longer overlap the later loads -- profiles/r04_experiments/sentinel_loop_ab.log.)
            if (interior) {
                const float w[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
                box_differences(w, r.ro, r0, r1, r2);
            }
        }
        if constexpr (PROF) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            t2 = __builtin_amdgcn_s_memtime();
            n_it++; n_int += __ballot(interior) != 0; n_leaf += __ballot(!interior) != 0;
            // how many DIFFERENT entries the wave's lanes hold in this iteration: one (the scalar-fetch case), two, three or four, more
            {
                unsigned long long left = __ballot(true);
                int groups = 0;
                while (left != 0ull && groups < 5) {
                    const int32_t c = __shfl(cur, __ffsll((long long)left) - 1);
                    left &= ~__ballot(cur == c);
                    groups++;
                }
                n_g1 += groups == 1; n_g2 += groups == 2; n_g34 += groups == 3 || groups == 4;
            }
        }
        if (interior) have = interior_apply<DEBUG, STK, OCT, kNeedPopValue>(r0, r1, r2, r3, r, hit.min, cur, stack, cnt);
        if constexpr (PROF) { __builtin_amdgcn_s_waitcnt(0); t3 = __builtin_amdgcn_s_memtime(); }
        bool accept = false;
        unsigned long long any_accept = 0ull;
        Candidate c;                                            // uninitialised on purpose, see Candidate
        const int slot = cur & kSlotMask;
        if (!interior) {                                        // leaf: contiguous triangle slots, raycast.cu:83-137
            const bool first = rem < 0;                         // first visit: decode the triangle count
            const int coded = (cur >> kSlotBits) & 31;
            rem = first ? coded : rem;
            if (first & (coded == 31)) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles: rare)
            if constexpr (DEBUG) {                              // (the instrumented kernel counts triangle tests: none for an empty leaf)
                if (rem > 0) accept = triangle_test<DEBUG, EX>(p, in, exact_uv, identity_inv, r, org, slot, hit.min, cnt, r0, r1, r2, r3, c);
            } else {
                // An empty leaf (degenerate splits only) holds no triangle to test: its "test" runs on whatever record sits at
                // the slot (always readable: the arrays are padded) and the result is masked -- one exec-mask region less
                // in every leaf iteration of every other scene.
                accept = triangle_test<DEBUG, EX>(p, in, exact_uv, identity_inv, r, org, slot, hit.min, cnt, r0, r1, r2, r3, c) & (rem > 0);
            }
            any_accept = __builtin_amdgcn_ballot_w64(accept);   // (asked here, where `accept` is a compare result, not a merged flag)
            rem--;
            have = rem > 0;
            cur = have ? cur + 1 : (kNeedPopValue ? kNeedPop : cur);    // next slot of the same leaf (the slot field never overflows)
            rem = have ? rem : -1;
        }
        if (any_accept != 0ull) {                               // (wave-level: most iterations accept nothing)
            hit.min = accept ? c.dist : hit.min;
            hit.slot = accept ? slot : hit.slot;
            hit.instance = accept ? inst_index : hit.instance;
            hit.u = accept ? (exact_uv ? c.uv.x : c.u) : hit.u;
            hit.v = accept ? (exact_uv ? c.uv.y : c.v) : hit.v;
            if constexpr (EX) { hit.loc.x = accept ? c.loc.x : hit.loc.x; hit.loc.y = accept ? c.loc.y : hit.loc.y; hit.loc.z = accept ? c.loc.z : hit.loc.z; }
            // raycast.cu:129-133: `if (lighting_pass && distance < light_distance) return hit_info;` -- the lane is done with
            // this cast: it takes the sentinel, which ends its loop at the bottom test (and cast_ray_ex skips its other instances)
            if constexpr (ANYHIT) {
                const bool done = accept & (c.dist < tmax);
                if constexpr (kNeedPopValue) cur = done ? kSentinel : cur;
                else {
                    // (EX keeps "must pop" as the flag: the lane leaves its leaf and finds nothing left but the sentinel when it pops next)
                    have = done ? false : have;
                    rem = done ? -1 : rem;
                    stack.sp = done ? 1 : stack.sp;
                }
            }
        }
        if constexpr (PROF) { __builtin_amdgcn_s_waitcnt(0); t0 = __builtin_amdgcn_s_memtime(); }
        // (kNeedPopValue: `have` is not read -- as a flag it is a lane mask that every branch of the loop has to merge into,
        // eight scalar instructions per iteration; as a value of `cur` it costs one select)
        if (kNeedPopValue ? cur == kNeedPop : !have) cur = stack.pop();     // raycast.cu:60-61 (the sentinel when nothing is left)
        // One latch for both ways round (popped / kept going): a convergent no-op that the optimiser may not clone.
        // Without it the two back edges are split into nested loops ("iterate while nobody pops" inside "pop"),
        // i.e. lanes that need a pop wait for every lane that does not: +50 % time on views with sky.
        __builtin_amdgcn_wave_barrier();
        if constexpr (PROF) {
            __builtin_amdgcn_s_waitcnt(0);
            c_mem += t2 - t1; c_int += t3 - t2; c_leaf += t0 - t3; c_pop += __builtin_amdgcn_s_memtime() - t0;
        }
    } while (cur != kSentinel);
    if constexpr (PROF) {
        if (p.trace) {                                          // the longest-lived lane's view of the wave
            unsigned long long v[10] = {c_pop, c_mem, c_int, c_leaf, n_it, n_int, n_leaf, n_g1, n_g2, n_g34};
            unsigned long long best = n_it;
            for (int o = 32; o > 0; o >>= 1) { unsigned long long x = __shfl_xor(best, o); best = x > best ? x : best; }
            const unsigned long long owner = __ballot(n_it == best);
            if ((int)(threadIdx.x & 63) == __ffsll((long long)owner) - 1) {
                unsigned long long* t = p.trace + (trace_workgroup() * (kPrimBlock / 64) + (threadIdx.x >> 6)) * 16 + 4;
                for (int k = 0; k < 10; k++) t[k] += v[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The traversal loop of the timed primary kernels, written in gfx950 assembly (the C++ loop above stays the
// reference form, the instrumented kernels' loop and the loop of every case this one does not take).
//
// Why: on this kernel every instruction costs the same, whatever unit executes it -- measured over four rounds of variants
// the frame time follows the TOTAL of instructions issued (vector + scalar + branch) at 0.67 us per million and frame
// (profiles/r05_experiments/instruction_issue_model.md) -- and a third of the compiler's loop is control flow: its structurizer
// wraps every condition in save / restore / skip sequences and keeps wave-uniform decisions in lane masks.  Written by hand an
// iteration needs two exec regions (the lanes at an interior node, the lanes at a triangle) with the push and the accepted
// hit as sub-regions, scalar branches for what is wave-uniform, and no flags.
// Scope: production primary rays (no counters), the LDS-only stack (plain or optimistic, see StackT), an instance without
// exact-uv mode (any pose: round 6 -- the accepted candidate's way back to world space is part of the loop, see the candidate
// block), a wave with a known sign octant (trace_instance's conditions for slab_oct).  Same arithmetic, instruction for instruction, as the C++ loop compiles to: the operations, their order and
// the IEEE division / square-root expansions are taken from the compiler's own output, so every bit of every result is
// the same (the parity tests compare this loop's frames and hit ids with the instrumented kernel's and the oracle's).
//
// Registers: v0..v15 the record, v16..v27 temporaries, s[48:63] the record of a wave-uniform fetch, s[30:45] and s[64:69] masks and
// scalars, s[46:47] the exec mask the loop was entered with; the ray, the hit and the stack state are operands.
// Hazards (gfx940 family): a VALU-written SGPR / VCC needs two wait states before a VALU reads it (none before a SALU read),
// four before v_div_fmas reads VCC; a transcendental result one before a non-transcendental VALU uses it.
// Round 6 rewrote the loop of round 5: the same decisions from fewer vector instructions -- masks that only the per-lane path reads are
// made there (and one of them by the scalar unit), "which child passes" is taken from the slab distances themselves instead of from
// FLT_MAX-patched copies of them, "the nearer child is next" is folded into one select, and the stack's top is kept as an LDS ADDRESS
// (push and pop add a constant to it instead of shifting an index).  No floating-point operation changed or moved; the round-5 text
// and the A/B against it: profiles/r06_experiments/asm_loop_v2.md.

// one interior node: v0..v11 hold box - origin, v12 / v13 the two child entries; exec = the lanes at this node.
// N* / F* = the registers holding the near / far plane of the axis for this octant (slab_oct's operand choice).
// pa = hit(a) and near(a) < hit.min, pb likewise: the reference's `dist < hit.min` on a distance that is FLT_MAX for a miss
// (BVHTree.hpp:40-54, raycast.cu:72-79) -- FLT_MAX < hit.min is false for every hit.min, so the mask is the same without the select;
// "a is the nearer" is only read where both pass, i.e. where both distances are the slab's own.  s[38:39] = pa, s[40:41] = pb,
// s[68:69] = near(a) < near(b), s[42:43] = the lanes that go on with a, vcc = the lanes that go on at all.
#define RT_ASM_INTERIOR(AXN, AXF, AYN, AYF, AZN, AZF, BXN, BXF, BYN, BYF, BZN, BZF) \
    "v_mul_f32 v16, " AXN ", %[dix]\n\t"  "v_mul_f32 v17, " AYN ", %[diy]\n\t"  "v_mul_f32 v18, " AZN ", %[diz]\n\t" \
    "v_mul_f32 v19, " AXF ", %[dix]\n\t"  "v_mul_f32 v20, " AYF ", %[diy]\n\t"  "v_mul_f32 v21, " AZF ", %[diz]\n\t" \
    "v_max3_f32 v16, v16, v17, v18\n\t"                 /* near of a */ \
    "v_min3_f32 v19, v19, v20, v21\n\t"                 /* far of a */ \
    "v_mul_f32 v22, " BXN ", %[dix]\n\t"  "v_mul_f32 v23, " BYN ", %[diy]\n\t"  "v_mul_f32 v24, " BZN ", %[diz]\n\t" \
    "v_mul_f32 v25, " BXF ", %[dix]\n\t"  "v_mul_f32 v26, " BYF ", %[diy]\n\t"  "v_mul_f32 v27, " BZF ", %[diz]\n\t" \
    "v_max3_f32 v22, v22, v23, v24\n\t"                 /* near of b */ \
    "v_min3_f32 v25, v25, v26, v27\n\t"                 /* far of b */ \
    "v_cmp_ge_f32_e32 vcc, v19, v16\n\t" \
    "v_cmp_lt_f32_e64 s[38:39], 0, v19\n\t" \
    "v_cmp_lt_f32_e64 s[44:45], v16, %[hmin]\n\t" \
    "v_cmp_ge_f32_e64 s[40:41], v25, v22\n\t" \
    "v_cmp_lt_f32_e64 s[42:43], 0, v25\n\t" \
    "v_cmp_lt_f32_e64 s[66:67], v22, %[hmin]\n\t" \
    "v_cmp_lt_f32_e64 s[68:69], v16, v22\n\t"           /* a is the nearer */ \
    "s_and_b64 vcc, vcc, s[38:39]\n\t" \
    "s_and_b64 s[40:41], s[40:41], s[42:43]\n\t" \
    "s_and_b64 s[38:39], vcc, s[44:45]\n\t"             /* pa */ \
    "s_and_b64 s[40:41], s[40:41], s[66:67]\n\t"        /* pb */ \
    "s_orn2_b64 s[42:43], s[68:69], s[40:41]\n\t" \
    "s_and_b64 s[44:45], s[38:39], s[40:41]\n\t"        /* both pass: one is pushed */ \
    "s_and_b64 s[42:43], s[42:43], s[38:39]\n\t"        /* a is next: it passes, and b does not or is the farther */ \
    "s_or_b64 vcc, s[38:39], s[40:41]\n\t"              /* any passes */ \
    "v_cndmask_b32_e64 v18, v13, v12, s[42:43]\n\t" \
    "s_and_saveexec_b64 s[38:39], s[44:45]\n\t" \
    "ds_write_b32 %[sa], %[tos]\n\t"                   /* the stack's top lives in a register: the one below it goes to LDS ... */ \
    "v_cmp_gt_i32_e64 s[44:45], %[lim], %[sa]\n\t"     /* the push fits (else it landed in the spare row and the lane stops, see StackT) */ \
    "v_add_u32_e32 %[sa], %[stride], %[sa]\n\t" \
    "v_cndmask_b32_e64 %[tos], v12, v13, s[68:69]\n\t" /* ... and the farther child becomes the top */ \
    "v_cndmask_b32_e64 v18, -2, v18, s[44:45]\n\t" \
    "s_or_b64 exec, exec, s[38:39]\n\t" \
    "v_cndmask_b32_e32 %[cur], -1, v18, vcc\n\t"        /* nothing passes: this lane pops */

// The pieces that differ between the plain loop and the VIEW loop (RtScene::ViewPool: interior records whose box words already are
// box - origin, `vdelta` bytes behind the records themselves):
//   UNI_OFFSET    s31 = byte offset of the wave's one entry            VEC_ADDR     v16 = byte offset of the lane's entry
//   UNI_INTERIOR  the interior step of a whole wave at one node         VEC_SUBS     box - origin of the lanes at interior nodes
#define RT_ASM_UNI_OFFSET_PLAIN \
    "s_lshl_b32 s31, s30, 6\n\t"
#define RT_ASM_UNI_OFFSET_VIEW \
    "s_cmp_lt_i32 s30, 0\n\t" \
    "s_cselect_b32 s38, 0, %[vdelta]\n\t"              /* (a triangle record is read where it always is) */ \
    "s_lshl_b32 s31, s30, 6\n\t" \
    "s_add_u32 s31, s31, s38\n\t"
#define RT_ASM_UNI_SUBS \
    "v_sub_f32_e32 v0, s48, %[rox]\n\t"  "v_sub_f32_e32 v1, s49, %[roy]\n\t"  "v_sub_f32_e32 v2, s50, %[roz]\n\t" \
    "v_sub_f32_e32 v3, s51, %[rox]\n\t"  "v_sub_f32_e32 v4, s52, %[roy]\n\t"  "v_sub_f32_e32 v5, s53, %[roz]\n\t" \
    "v_sub_f32_e32 v6, s54, %[rox]\n\t"  "v_sub_f32_e32 v7, s55, %[roy]\n\t"  "v_sub_f32_e32 v8, s56, %[roz]\n\t" \
    "v_sub_f32_e32 v9, s57, %[rox]\n\t"  "v_sub_f32_e32 v10, s58, %[roy]\n\t" "v_sub_f32_e32 v11, s59, %[roz]\n\t"
#define RT_ASM_VEC_ADDR_PLAIN \
    "v_lshlrev_b32_e32 v16, 6, %[cur]\n\t"
#define RT_ASM_VEC_ADDR_VIEW \
    "v_mov_b32_e32 v17, %[vdelta]\n\t" \
    "v_cndmask_b32_e64 v17, 0, v17, s[64:65]\n\t"      /* lanes at an interior node read the frame's view of it */ \
    "v_lshl_add_u32 v16, %[cur], 6, v17\n\t"
#define RT_ASM_VEC_SUBS \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_sub_f32_e32 v0, v0, %[rox]\n\t"  "v_sub_f32_e32 v1, v1, %[roy]\n\t"  "v_sub_f32_e32 v2, v2, %[roz]\n\t" \
    "v_sub_f32_e32 v3, v3, %[rox]\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_sub_f32_e32 v4, v4, %[roy]\n\t"  "v_sub_f32_e32 v5, v5, %[roz]\n\t" \
    "v_sub_f32_e32 v6, v6, %[rox]\n\t"  "v_sub_f32_e32 v7, v7, %[roy]\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_sub_f32_e32 v8, v8, %[roz]\n\t" \
    "v_sub_f32_e32 v9, v9, %[rox]\n\t"  "v_sub_f32_e32 v10, v10, %[roy]\n\t" "v_sub_f32_e32 v11, v11, %[roz]\n\t"

// POPS (the samples-only extension kernel counts node pops per lane): one more per interior node, one per leaf arrived at
#define RT_ASM_POPS_INTERIOR "v_add_u32_e32 %[pops], 1, %[pops]\n\t"
#define RT_ASM_POPS_LEAF \
    "v_cndmask_b32_e64 v17, 0, 1, vcc\n\t"             /* (vcc = first triangle of this leaf, two instructions old) */ \
    "v_add_u32_e32 %[pops], %[pops], v17\n\t"

// LOC (the bounce kernel's primary ray): the accepted candidate's point on its plane, in mesh space -- the caller turns it into the
// world-space hit location with the reference's own sequence (raycast.cu:98-104), once, for the hit that was kept
// ANYHIT (a shadow ray of the extension kernel or a query of rt_occluded, raycast.cu:129-133: the cast returns at its first accepted hit
// below the lane's light distance %[tmax], a VGPR: FLT_MAX for shadow rays, per ray for rt_occluded): s[66:67] = the lanes
// that accepted such a hit in this triangle step (cleared at the step's start, set in the accepted-candidate block where exec = those
// lanes and v21 = the distance); they take the sentinel after the step's own bookkeeping and leave the loop at the latch
#define RT_ASM_ANYHIT_CLEAR "s_mov_b64 s[66:67], 0\n\t"
#define RT_ASM_ANYHIT_MARK "v_cmp_lt_f32_e64 s[66:67], v21, %[tmax]\n\t"
#define RT_ASM_ANYHIT_LEAVE "v_cndmask_b32_e64 %[cur], %[cur], -2, s[66:67]\n\t"
#define RT_ASM_LOC "v_mov_b32_e32 %[px], v18\n\tv_mov_b32_e32 %[py], v19\n\tv_mov_b32_e32 %[pz], v20\n\t"

// Few TAKEN branches on the common paths -- a taken branch restarts the wave's instruction fetch.  The count lookup of a leaf above
// 30 triangles sits out of line (.Lrt_long: the branch over it was taken at almost every triangle), and the wave-uniform interior step
// ends in its own copy of the pop / latch block instead of a branch to the shared one (profiles/r06_experiments/asm_loop_v2.md).
#define RT_ASM_POP \
    "v_subrev_u32_e32 %[sa], %[stride], %[sa]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t"                         /* (the top's reload of an earlier pop: long done) */ \
    "v_mov_b32_e32 %[cur], %[tos]\n\t"                 /* the popped entry is in a register: the lane goes on at once ... */ \
    "ds_read_b32 %[tos], %[sa]\n\t"                    /* ... and the new top arrives while it works on it */
#define RT_ASM_UNI_TAIL \
    "v_cmp_eq_u32_e32 vcc, -1, %[cur]\n\t" \
    "s_and_saveexec_b64 s[36:37], vcc\n\t" \
    "s_cbranch_execz .Lrt_latch_u%=\n\t" \
    RT_ASM_POP \
    ".Lrt_latch_u%=:\n\t" \
    "s_or_b64 exec, exec, s[36:37]\n\t" \
    "v_cmp_ne_u32_e32 vcc, -2, %[cur]\n\t" \
    "s_and_b64 exec, exec, vcc\n\t" \
    "s_cbranch_execnz .Lrt_top%=\n\t" \
    "s_branch .Lrt_exit%=\n\t"
// s[64:65] = the lanes at an interior node, s[34:35] = the lanes at a triangle: read by the per-lane path only, and made there (the
// second one is exec without the first: an entry of a live lane is a node or a triangle).  VEC_ADDR_VIEW reads s[64:65] two
// instructions later.
#define RT_ASM_LOOP_TEXT(COUNT_TEXT, POPS_INT, POPS_LEAF, LOC_TEXT, LEAF_TAIL, UNI_OFFSET, UNI_INTERIOR, VEC_ADDR, VEC_SUBS, AXN, AXF, AYN, AYF, AZN, AZF, BXN, BXF, BYN, BYF, BZN, BZF) \
    "s_mov_b64 s[46:47], exec\n\t" \
    ".Lrt_top%=:\n\t" \
    COUNT_TEXT \
    "v_readfirstlane_b32 s30, %[cur]\n\t" \
    "s_nop 1\n\t"                                       /* (a vector read of s30 after v_readfirstlane: two wait states) */ \
    "v_cmp_ne_u32_e32 vcc, s30, %[cur]\n\t" \
    "s_cbranch_vccnz .Lrt_vector%=\n\t" \
    /* ---- every lane holds the same entry: the record comes through the scalar cache */ \
    UNI_OFFSET \
    "s_load_dwordx16 s[48:63], %[rec], s31\n\t" \
    "s_cmp_lt_i32 s30, 0\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_cbranch_scc1 .Lrt_one_leaf%=\n\t" \
    "v_mov_b32_e32 v12, s60\n\t" \
    "v_mov_b32_e32 v13, s61\n\t" \
    POPS_INT \
    UNI_INTERIOR \
    RT_ASM_UNI_TAIL \
    ".Lrt_one_leaf%=:\n\t" \
    "v_mov_b32_e32 v0, s48\n\t"  "v_mov_b32_e32 v1, s49\n\t"  "v_mov_b32_e32 v2, s50\n\t"  "v_mov_b32_e32 v3, s51\n\t" \
    "v_mov_b32_e32 v4, s52\n\t"  "v_mov_b32_e32 v5, s53\n\t"  "v_mov_b32_e32 v6, s54\n\t"  "v_mov_b32_e32 v7, s55\n\t" \
    "v_mov_b32_e32 v8, s56\n\t"  "v_mov_b32_e32 v9, s57\n\t"  "v_mov_b32_e32 v10, s58\n\t" "v_mov_b32_e32 v11, s59\n\t" \
    "v_mov_b32_e32 v12, s60\n\t" "v_mov_b32_e32 v13, s61\n\t" "v_mov_b32_e32 v14, s62\n\t" "v_mov_b32_e32 v15, s63\n\t" \
    "s_mov_b64 s[36:37], exec\n\t" \
    "s_branch .Lrt_leaf%=\n\t" \
    /* ---- lanes hold different entries: one 64-byte record per lane, node or triangle, from one array */ \
    ".Lrt_vector%=:\n\t" \
    "v_cmp_lt_i32_e64 s[64:65], -1, %[cur]\n\t" \
    "s_andn2_b64 s[34:35], exec, s[64:65]\n\t" \
    VEC_ADDR \
    "global_load_dwordx4 v[0:3], v16, %[rec]\n\t" \
    "global_load_dwordx4 v[4:7], v16, %[rec] offset:16\n\t" \
    "global_load_dwordx4 v[8:11], v16, %[rec] offset:32\n\t" \
    "global_load_dwordx4 v[12:15], v16, %[rec] offset:48\n\t" \
    "s_and_saveexec_b64 s[36:37], s[64:65]\n\t" \
    "s_cbranch_execz .Lrt_leaf_lanes%=\n\t" \
    POPS_INT \
    VEC_SUBS \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    RT_ASM_INTERIOR(AXN, AXF, AYN, AYF, AZN, AZF, BXN, BXF, BYN, BYF, BZN, BZF) \
    ".Lrt_leaf_lanes%=:\n\t" \
    "s_or_b64 exec, exec, s[36:37]\n\t" \
    "s_and_saveexec_b64 s[36:37], s[34:35]\n\t" \
    "s_cbranch_execz .Lrt_leaf_done%=\n\t" \
    /* ---- one triangle of a leaf (exec = the lanes at one; s[36:37] = the mask to return to) */ \
    ".Lrt_leaf%=:\n\t" \
    "v_bfe_u32 v16, %[cur], 26, 5\n\t"                  /* the count coded in the entry */ \
    "v_cmp_gt_i32_e32 vcc, 0, %[rem]\n\t"               /* first triangle of this leaf */ \
    "v_cmp_eq_u32_e64 s[38:39], 31, v16\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cndmask_b32_e32 %[rem], %[rem], v16, vcc\n\t" \
    POPS_LEAF \
    "s_and_b64 s[38:39], s[38:39], vcc\n\t"             /* a leaf of more than 30 triangles: its count is in leaf_count */ \
    "s_cbranch_scc1 .Lrt_long%=\n\t" \
    ".Lrt_short%=:\n\t" \
    /* TrianglePrimitive::ray_intersect: denom = rd . n, tt = ((v0 - ro) . n) / denom */ \
    "v_mul_f32_e32 v16, %[rdx], v3\n\t" \
    "v_mul_f32_e32 v17, %[rdy], v4\n\t" \
    "v_add_f32_e32 v16, v16, v17\n\t" \
    "v_mul_f32_e32 v17, %[rdz], v5\n\t" \
    "v_add_f32_e32 v16, v16, v17\n\t"                   /* denom */ \
    "v_sub_f32_e32 v17, v0, %[rox]\n\t" \
    "v_sub_f32_e32 v18, v1, %[roy]\n\t" \
    "v_sub_f32_e32 v19, v2, %[roz]\n\t" \
    "v_mul_f32_e32 v17, v17, v3\n\t" \
    "v_mul_f32_e32 v18, v18, v4\n\t" \
    "v_add_f32_e32 v17, v17, v18\n\t" \
    "v_mul_f32_e32 v18, v19, v5\n\t" \
    "v_add_f32_e32 v17, v17, v18\n\t"                   /* numerator */ \
    "v_div_scale_f32 v18, s[38:39], v16, v16, v17\n\t" \
    "v_rcp_f32_e32 v19, v18\n\t" \
    "v_cmp_nlt_f32_e64 s[40:41], |v16|, %[eps]\n\t"     /* !(|denom| < 1e-6) */ \
    "v_cmp_gt_f32_e64 s[42:43], 0, v16\n\t"             /* denom < 0: the only candidates that can be accepted */ \
    /* no lane of the wave holds a triangle that faces its ray: the rest of the test -- the division, the point on the plane, the \
       barycentrics -- is skipped for the whole wave */ \
    "s_and_b64 s[40:41], s[40:41], s[42:43]\n\t" \
    "s_cbranch_scc0 .Lrt_next_triangle%=\n\t" \
    "v_fma_f32 v20, -v18, v19, 1.0\n\t" \
    "v_fmac_f32_e32 v19, v20, v19\n\t" \
    "v_div_scale_f32 v20, vcc, v17, v16, v17\n\t" \
    "v_mul_f32_e32 v21, v20, v19\n\t" \
    "v_fma_f32 v22, -v18, v21, v20\n\t" \
    "v_fmac_f32_e32 v21, v22, v19\n\t" \
    "v_fma_f32 v18, -v18, v21, v20\n\t" \
    "v_div_fmas_f32 v18, v18, v19, v21\n\t" \
    "v_div_fixup_f32 v17, v18, v16, v17\n\t"            /* tt */ \
    "v_mul_f32_e32 v18, %[rdx], v17\n\t" \
    "v_mul_f32_e32 v19, %[rdy], v17\n\t" \
    "v_mul_f32_e32 v20, %[rdz], v17\n\t" \
    "v_cmp_nlt_f32_e64 s[42:43], v17, 0\n\t"            /* !(tt < 0) */ \
    "v_add_f32_e32 v18, %[rox], v18\n\t"                /* the point on the plane */ \
    "v_add_f32_e32 v19, %[roy], v19\n\t" \
    "v_add_f32_e32 v20, %[roz], v20\n\t" \
    "s_and_b64 s[40:41], s[40:41], s[42:43]\n\t" \
    "v_cmp_neq_f32_e32 vcc, 0x7f7fffff, v18\n\t"        /* raycast.cu:91 */ \
    /* TrianglePrimitive::point_inside */ \
    "v_sub_f32_e32 v21, v18, v0\n\t" \
    "v_sub_f32_e32 v22, v19, v1\n\t" \
    "v_sub_f32_e32 v23, v20, v2\n\t" \
    "s_and_b64 s[40:41], s[40:41], vcc\n\t" \
    "v_mul_f32_e32 v24, v6, v21\n\t" \
    "v_mul_f32_e32 v25, v7, v22\n\t" \
    "v_add_f32_e32 v24, v24, v25\n\t" \
    "v_mul_f32_e32 v25, v8, v23\n\t" \
    "v_add_f32_e32 v24, v24, v25\n\t"                   /* dot02 */ \
    "v_mul_f32_e32 v25, v9, v21\n\t" \
    "v_mul_f32_e32 v26, v10, v22\n\t" \
    "v_add_f32_e32 v25, v25, v26\n\t" \
    "v_mul_f32_e32 v26, v11, v23\n\t" \
    "v_add_f32_e32 v25, v25, v26\n\t"                   /* dot12 */ \
    "v_mul_f32_e32 v26, v14, v24\n\t" \
    "v_mul_f32_e32 v27, v13, v25\n\t" \
    "v_sub_f32_e32 v26, v26, v27\n\t" \
    "v_mul_f32_e32 v26, v26, v15\n\t"                   /* u */ \
    "v_mul_f32_e32 v27, v12, v25\n\t" \
    "v_mul_f32_e32 v21, v13, v24\n\t" \
    "v_sub_f32_e32 v27, v27, v21\n\t" \
    "v_mul_f32_e32 v27, v27, v15\n\t"                   /* v */ \
    "v_cmp_le_f32_e32 vcc, 0, v26\n\t" \
    "v_cmp_le_f32_e64 s[42:43], 0, v27\n\t" \
    "v_add_f32_e32 v21, v26, v27\n\t" \
    "s_and_b64 s[40:41], s[40:41], vcc\n\t" \
    "v_cmp_ge_f32_e32 vcc, 1.0, v21\n\t" \
    "s_and_b64 s[40:41], s[40:41], s[42:43]\n\t" \
    "s_and_b64 s[40:41], s[40:41], vcc\n\t"             /* a candidate inside its triangle */ \
    "s_and_saveexec_b64 s[44:45], s[40:41]\n\t" \
    "s_cbranch_execz .Lrt_no_candidate%=\n\t" \
    /* its world-space location, raycast.cu:98-104: (pt * scale - inv_pose.xyz) rotated by q_inv_pose.  For an instance with scale 1 and the \
       identity quaternion -- translated or not: the common case, and the reference's own scene (kernel.cu:209-240) -- the product and the rotation \
       return their operand (up to the sign of a zero, which the squares below cannot see) and only the subtraction is left; any other \
       instance takes the whole sequence, out of line behind a scalar branch (.Lrt_general, after the loop) */ \
    "s_cmp_lg_u64 %[ip], 0\n\t" \
    "s_cbranch_scc1 .Lrt_general%=\n\t" \
    "v_subrev_f32_e32 v21, %[tx], v18\n\t" \
    "v_subrev_f32_e32 v22, %[ty], v19\n\t" \
    "v_subrev_f32_e32 v23, %[tz], v20\n\t" \
    ".Lrt_have_loc%=:\n\t" \
    /* its distance from the ray's world origin */ \
    "v_subrev_f32_e32 v21, %[orgx], v21\n\t" \
    "v_subrev_f32_e32 v22, %[orgy], v22\n\t" \
    "v_subrev_f32_e32 v23, %[orgz], v23\n\t" \
    "v_mul_f32_e32 v21, v21, v21\n\t" \
    "v_mul_f32_e32 v22, v22, v22\n\t" \
    "v_add_f32_e32 v21, v21, v22\n\t" \
    "v_mul_f32_e32 v22, v23, v23\n\t" \
    "v_add_f32_e32 v21, v21, v22\n\t" \
    "s_mov_b32 s31, 0xf800000\n\t"                      /* sqrtf, as the compiler expands it */ \
    "s_movk_i32 s30, 0x260\n\t" \
    "v_mul_f32_e32 v22, 0x4f800000, v21\n\t" \
    "v_cmp_gt_f32_e32 vcc, s31, v21\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_e32 v21, v21, v22, vcc\n\t" \
    "v_sqrt_f32_e32 v22, v21\n\t" \
    "s_nop 0\n\t" \
    "v_add_u32_e32 v23, -1, v22\n\t" \
    "v_fma_f32 v24, -v23, v22, v21\n\t" \
    "v_cmp_ge_f32_e64 s[38:39], 0, v24\n\t" \
    "v_add_u32_e32 v24, 1, v22\n\t" \
    "s_nop 0\n\t" \
    "v_cndmask_b32_e64 v23, v22, v23, s[38:39]\n\t" \
    "v_fma_f32 v22, -v24, v22, v21\n\t" \
    "v_cmp_lt_f32_e64 s[38:39], 0, v22\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_e64 v22, v23, v24, s[38:39]\n\t" \
    "v_mul_f32_e32 v23, 0x37800000, v22\n\t" \
    "v_cndmask_b32_e32 v22, v22, v23, vcc\n\t" \
    "v_cmp_class_f32_e64 vcc, v21, s30\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_e32 v21, v22, v21, vcc\n\t"          /* distance */ \
    /* raycast.cu:107-109: accepted when nothing was hit yet or this is closer (denom < 0 is part of the candidate mask) */ \
    "v_cmp_eq_f32_e32 vcc, 0x7f7fffff, %[hmin]\n\t" \
    "v_cmp_lt_f32_e64 s[38:39], v21, %[hmin]\n\t" \
    "v_cmp_lt_i32_e64 s[42:43], 0, %[rem]\n\t"          /* (an empty leaf holds no triangle) */ \
    "s_or_b64 vcc, vcc, s[38:39]\n\t" \
    "s_and_b64 vcc, vcc, s[42:43]\n\t" \
    "s_and_b64 exec, exec, vcc\n\t" \
    "v_mov_b32_e32 %[hmin], v21\n\t" \
    "v_and_b32_e32 %[hslot], 0x3ffffff, %[cur]\n\t" \
    "v_mov_b32_e32 %[hinst], %[inst]\n\t" \
    "v_mov_b32_e32 %[hu], v26\n\t" \
    "v_mov_b32_e32 %[hv], v27\n\t" \
    LOC_TEXT \
    ".Lrt_no_candidate%=:\n\t" \
    "s_or_b64 exec, exec, s[44:45]\n\t" \
    ".Lrt_next_triangle%=:\n\t" \
    /* next triangle of the leaf, or a pop */ \
    "v_add_u32_e32 %[rem], -1, %[rem]\n\t" \
    "v_add_u32_e32 v16, 1, %[cur]\n\t" \
    "v_cmp_lt_i32_e32 vcc, 0, %[rem]\n\t" \
    "s_nop 1\n\t" \
    "v_cndmask_b32_e32 %[cur], -1, v16, vcc\n\t" \
    "v_cndmask_b32_e32 %[rem], -1, %[rem], vcc\n\t" \
    LEAF_TAIL \
    ".Lrt_leaf_done%=:\n\t" \
    "s_or_b64 exec, exec, s[36:37]\n\t" \
    /* ---- raycast.cu:60-61: lanes with nothing to go on with pop (the sentinel when nothing is left) */ \
    ".Lrt_pop%=:\n\t" \
    "v_cmp_eq_u32_e32 vcc, -1, %[cur]\n\t" \
    "s_and_saveexec_b64 s[36:37], vcc\n\t" \
    "s_cbranch_execz .Lrt_latch%=\n\t" \
    RT_ASM_POP \
    ".Lrt_latch%=:\n\t" \
    "s_or_b64 exec, exec, s[36:37]\n\t" \
    "v_cmp_ne_u32_e32 vcc, -2, %[cur]\n\t" \
    "s_and_b64 exec, exec, vcc\n\t"                     /* lanes that popped the sentinel are done */ \
    "s_cbranch_execnz .Lrt_top%=\n\t" \
    ".Lrt_exit%=:\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t"                         /* (the last pop's reload of the top) */ \
    "s_mov_b64 exec, s[46:47]\n\t" \
    "s_branch .Lrt_end%=\n\t" \
    /* ---- out of line: mesh -> world of an accepted candidate for an instance that is scaled or rotated (raycast.cu:98-104 with \
       apply_quat of transforms.hpp:165-176 written out: the same products and sums in the same association, no contraction).  The \
       record's registers v0..v7 are free here (the triangle test is over), and so are s[48:63]: the instance's inverse pose comes \
       through the scalar cache where it is needed instead of sitting in ten scalar registers around the loop */ \
    ".Lrt_general%=:\n\t" \
    "s_load_dwordx4 s[48:51], %[ip], 0x20\n\t"         /* DevInstance::q_inv_pose */ \
    "s_load_dwordx2 s[52:53], %[ip], 0x58\n\t"         /* DevInstance::scale x y */ \
    "s_load_dword s54, %[ip], 0x60\n\t"                /* DevInstance::scale z */ \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mul_f32_e32 v0, s52, v18\n\t" \
    "v_mul_f32_e32 v1, s53, v19\n\t" \
    "v_mul_f32_e32 v2, s54, v20\n\t" \
    "v_subrev_f32_e32 v0, %[tx], v0\n\t" \
    "v_subrev_f32_e32 v1, %[ty], v1\n\t" \
    "v_subrev_f32_e32 v2, %[tz], v2\n\t" \
    "v_mul_f32_e64 v3, -v0, s49\n\t"                   /* a = -v.x * q.y - v.y * q.z - v.z * q.w */ \
    "v_mul_f32_e32 v4, s50, v1\n\t" \
    "v_sub_f32_e32 v3, v3, v4\n\t" \
    "v_mul_f32_e32 v4, s51, v2\n\t" \
    "v_sub_f32_e32 v3, v3, v4\n\t" \
    "v_mul_f32_e32 v4, s48, v0\n\t"                    /* b = v.x * q.x + v.y * q.w - v.z * q.z */ \
    "v_mul_f32_e32 v5, s51, v1\n\t" \
    "v_add_f32_e32 v4, v4, v5\n\t" \
    "v_mul_f32_e32 v5, s50, v2\n\t" \
    "v_sub_f32_e32 v4, v4, v5\n\t" \
    "v_mul_f32_e32 v5, s48, v1\n\t"                    /* c = v.y * q.x + v.z * q.y - v.x * q.w */ \
    "v_mul_f32_e32 v6, s49, v2\n\t" \
    "v_add_f32_e32 v5, v5, v6\n\t" \
    "v_mul_f32_e32 v6, s51, v0\n\t" \
    "v_sub_f32_e32 v5, v5, v6\n\t" \
    "v_mul_f32_e32 v6, s48, v2\n\t"                    /* d = v.z * q.x + v.x * q.z - v.y * q.y */ \
    "v_mul_f32_e32 v7, s50, v0\n\t" \
    "v_add_f32_e32 v6, v6, v7\n\t" \
    "v_mul_f32_e32 v7, s49, v1\n\t" \
    "v_sub_f32_e32 v6, v6, v7\n\t" \
    "v_mul_f32_e32 v21, s48, v4\n\t"                   /* x = q.x * b - q.y * a - q.z * d + q.w * c */ \
    "v_mul_f32_e32 v7, s49, v3\n\t" \
    "v_sub_f32_e32 v21, v21, v7\n\t" \
    "v_mul_f32_e32 v7, s50, v6\n\t" \
    "v_sub_f32_e32 v21, v21, v7\n\t" \
    "v_mul_f32_e32 v7, s51, v5\n\t" \
    "v_add_f32_e32 v21, v21, v7\n\t" \
    "v_mul_f32_e32 v22, s48, v5\n\t"                   /* y = q.x * c - q.z * a - q.w * b + q.y * d */ \
    "v_mul_f32_e32 v7, s50, v3\n\t" \
    "v_sub_f32_e32 v22, v22, v7\n\t" \
    "v_mul_f32_e32 v7, s51, v4\n\t" \
    "v_sub_f32_e32 v22, v22, v7\n\t" \
    "v_mul_f32_e32 v7, s49, v6\n\t" \
    "v_add_f32_e32 v22, v22, v7\n\t" \
    "v_mul_f32_e32 v23, s48, v6\n\t"                   /* z = q.x * d - q.w * a - q.y * c + q.z * b */ \
    "v_mul_f32_e32 v7, s51, v3\n\t" \
    "v_sub_f32_e32 v23, v23, v7\n\t" \
    "v_mul_f32_e32 v7, s49, v5\n\t" \
    "v_sub_f32_e32 v23, v23, v7\n\t" \
    "v_mul_f32_e32 v7, s50, v4\n\t" \
    "v_add_f32_e32 v23, v23, v7\n\t" \
    "s_branch .Lrt_have_loc%=\n\t" \
    /* ---- out of line: the count of a leaf of more than 30 triangles */ \
    ".Lrt_long%=:\n\t" \
    "s_and_saveexec_b64 s[40:41], s[38:39]\n\t" \
    "v_and_b32_e32 v17, 0x3ffffff, %[cur]\n\t" \
    "v_lshlrev_b32_e32 v17, 2, v17\n\t" \
    "global_load_dword %[rem], v17, %[lc]\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "s_or_b64 exec, exec, s[40:41]\n\t" \
    "s_branch .Lrt_short%=\n\t" \
    ".Lrt_end%=:\n\t"

// (the byte offsets .Lrt_general reads the instance record at)
static_assert(offsetof(DevInstance, q_inv_pose) == 0x20 && offsetof(DevInstance, scale) == 0x58 && sizeof(DevInstance) % 16 == 0, "DevInstance layout");

// ORGV: the ray's world origin differs per lane (the ray queries' rays): vector operands, and never a VIEW
template <int OCT, bool COUNT, int ROW_SHIFT, bool VIEW, bool POPS, bool LOC, bool ORGV = false, bool ANYHIT = false>  // ROW_SHIFT = log2 of the bytes between two entries of a lane's LDS stack column
__device__ __forceinline__ void trace_loop_asm(const RenderParams& p, int inst_index, const MeshRay& r, V3 org, lds_int* column, int lds_depth,
                                               int32_t& cur, int32_t& sp, Hit& hit, int& wave_iters, uint32_t vdelta, int& pops, V3& point,
                                               V3 back, const DevInstance* general, float tmax = FLT_MAX)
{
    // back = DevInstance::inv_pose_xyz (wave-uniform: scalar operands); general = the instance when its mesh -> world transform scales or
    // rotates (the candidate block then reads scale and q_inv_pose through the scalar cache), null when it only translates
    static_assert(!LOC || POPS, "the hit point is kept for the extension kernel, which counts pops");
    static_assert(!(ORGV && VIEW) && !(ANYHIT && (LOC || !POPS || !ORGV)), "secondary rays: no view; a shadow ray keeps no location");
    int32_t rem = -1;
    // the stack pointer as the LDS address of the next free row of the lane's column, and the address of the first row that is not there
    // -- as a SCALAR: a column starts less than one row pitch behind its wave's first column (4 bytes per lane), so `row < depth` is
    // `address < first column of the wave + depth * pitch` for every lane
    lds_int* sa = column + (sp << (ROW_SHIFT - 2));
    // (scalar arithmetic on the first active lane's column: a per-lane `column - lane` would be one more value to keep across the loop)
    const int32_t limit = __builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(size_t)column) - 4 * (int32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true)) +
                          (lds_depth << ROW_SHIFT);
#define RT_ASM_STACK_OUT [sa] "+v"(sa)
#define RT_ASM_STACK_IN [lim] "s"(limit), [stride] "n"(1 << ROW_SHIFT)
    int32_t tos = kSentinel;                                    // the stack's top entry (row 0 of the LDS column holds a second sentinel, so
                                                                // that the last pop's reload reads a row that exists and leaves sp == 0)
    const float eps = __int_as_float(0x358637be);
#define RT_ASM_OUT_PLAIN
#define RT_ASM_OUT_POPS , [pops] "+v"(pops)           /* (only the variants that count pops hold a register for them) */
#define RT_ASM_OUT_LOC , [pops] "+v"(pops), [px] "+v"(point.x), [py] "+v"(point.y), [pz] "+v"(point.z)
#define RT_ASM_OUT_ANYHIT , [pops] "+v"(pops), [tmax] "+v"(tmax)     /* (only read; in this list it costs the other variants no register) */
#define RT_ASM_GO(TEXT) RT_ASM_GO2(TEXT, RT_ASM_OUT_PLAIN)
#define RT_ASM_GO2(TEXT, ...)        /* (... = more output operands, with their leading comma, or nothing) */ \
    asm volatile(TEXT \
                 : [cur] "+v"(cur), RT_ASM_STACK_OUT, [rem] "+v"(rem), [tos] "+v"(tos), [hmin] "+v"(hit.min), [hslot] "+v"(hit.slot), [hinst] "+v"(hit.instance), \
                   [hu] "+v"(hit.u), [hv] "+v"(hit.v), [iters] "+s"(wave_iters) __VA_ARGS__ \
                 : [rox] "v"(r.ro.x), [roy] "v"(r.ro.y), [roz] "v"(r.ro.z), [rdx] "v"(r.rd.x), [rdy] "v"(r.rd.y), [rdz] "v"(r.rd.z), \
                   [dix] "v"(r.dinv.x), [diy] "v"(r.dinv.y), [diz] "v"(r.dinv.z), RT_ASM_STACK_IN, \
                   [rec] "s"(p.records), [lc] "s"(p.leaf_count), [orgx] RT_ASM_ORG_C(org.x), [orgy] RT_ASM_ORG_C(org.y), [orgz] RT_ASM_ORG_C(org.z), \
                   [inst] "s"(inst_index), [eps] "s"(eps), [vdelta] "s"(vdelta), \
                   [tx] "s"(back.x), [ty] "s"(back.y), [tz] "s"(back.z), [ip] "s"(general) \
                 : "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", \
                   "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", \
                   "s30", "s31", "s64", "s65", "s34", "s35", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", \
                   "s66", "s67", "s68", "s69", "vcc", "scc", "memory")
#define RT_ASM_COUNT "s_add_u32 %[iters], %[iters], 1\n\t"
#define RT_ASM_NOCOUNT ""
#define RT_ASM_ARGS(...) __VA_ARGS__
    // VN = the registers of the record's planes as the per-lane fetch leaves them (x: v0 / v3 for box a, v6 / v9 for box b; y: v1 / v4,
    // v7 / v10; z: v2 / v5, v8 / v11 -- min, max), SN = the scalar registers a wave-uniform fetch leaves them in (s48 ..): per axis
    // (near, far) for this octant -- bit k of OCT set = direction component k negative = the max plane is the near one (slab_oct).
#define RT_ASM_VARIANT(CT, PI, PL, LT, TL, OUT, VN, SN) \
    if constexpr (VIEW) RT_ASM_GO2(RT_ASM_LOOP_TEXT(CT, PI, PL, LT, TL, RT_ASM_UNI_OFFSET_VIEW, RT_ASM_INTERIOR(SN), RT_ASM_VEC_ADDR_VIEW, "", VN), OUT); \
    else RT_ASM_GO2(RT_ASM_LOOP_TEXT(CT, PI, PL, LT, TL, RT_ASM_UNI_OFFSET_PLAIN, RT_ASM_UNI_SUBS RT_ASM_INTERIOR(VN), RT_ASM_VEC_ADDR_PLAIN, RT_ASM_VEC_SUBS, VN), OUT)
    // (COUNT -- the tile cost of single-frame primary launches -- and POPS -- the extension kernel's pop plane -- never meet)
#define RT_ASM_CASE(N, VN, SN) \
    if constexpr (OCT == N) { if constexpr (LOC) { RT_ASM_VARIANT(RT_ASM_NOCOUNT, RT_ASM_POPS_INTERIOR, RT_ASM_POPS_LEAF, RT_ASM_LOC, "", RT_ASM_OUT_LOC, RT_ASM_ARGS(VN), RT_ASM_ARGS(SN)); } \
                              RT_ASM_CASE_ANYHIT(RT_ASM_ARGS(VN), RT_ASM_ARGS(SN)) \
                              else if constexpr (POPS) { RT_ASM_VARIANT(RT_ASM_NOCOUNT, RT_ASM_POPS_INTERIOR, RT_ASM_POPS_LEAF, "", "", RT_ASM_OUT_POPS, RT_ASM_ARGS(VN), RT_ASM_ARGS(SN)); } \
                              else if constexpr (COUNT) { RT_ASM_VARIANT(RT_ASM_COUNT, "", "", "", "", RT_ASM_OUT_PLAIN, RT_ASM_ARGS(VN), RT_ASM_ARGS(SN)); } \
                              else { RT_ASM_VARIANT(RT_ASM_NOCOUNT, "", "", "", "", RT_ASM_OUT_PLAIN, RT_ASM_ARGS(VN), RT_ASM_ARGS(SN)); } }
#define RT_ASM_ALL_CASES \
    RT_ASM_CASE(0, RT_ASM_ARGS("v0", "v3", "v1", "v4", "v2", "v5", "v6", "v9", "v7", "v10", "v8", "v11"), RT_ASM_ARGS("s48", "s51", "s49", "s52", "s50", "s53", "s54", "s57", "s55", "s58", "s56", "s59")) \
    RT_ASM_CASE(1, RT_ASM_ARGS("v3", "v0", "v1", "v4", "v2", "v5", "v9", "v6", "v7", "v10", "v8", "v11"), RT_ASM_ARGS("s51", "s48", "s49", "s52", "s50", "s53", "s57", "s54", "s55", "s58", "s56", "s59")) \
    RT_ASM_CASE(2, RT_ASM_ARGS("v0", "v3", "v4", "v1", "v2", "v5", "v6", "v9", "v10", "v7", "v8", "v11"), RT_ASM_ARGS("s48", "s51", "s52", "s49", "s50", "s53", "s54", "s57", "s58", "s55", "s56", "s59")) \
    RT_ASM_CASE(3, RT_ASM_ARGS("v3", "v0", "v4", "v1", "v2", "v5", "v9", "v6", "v10", "v7", "v8", "v11"), RT_ASM_ARGS("s51", "s48", "s52", "s49", "s50", "s53", "s57", "s54", "s58", "s55", "s56", "s59")) \
    RT_ASM_CASE(4, RT_ASM_ARGS("v0", "v3", "v1", "v4", "v5", "v2", "v6", "v9", "v7", "v10", "v11", "v8"), RT_ASM_ARGS("s48", "s51", "s49", "s52", "s53", "s50", "s54", "s57", "s55", "s58", "s59", "s56")) \
    RT_ASM_CASE(5, RT_ASM_ARGS("v3", "v0", "v1", "v4", "v5", "v2", "v9", "v6", "v7", "v10", "v11", "v8"), RT_ASM_ARGS("s51", "s48", "s49", "s52", "s53", "s50", "s57", "s54", "s55", "s58", "s59", "s56")) \
    RT_ASM_CASE(6, RT_ASM_ARGS("v0", "v3", "v4", "v1", "v5", "v2", "v6", "v9", "v10", "v7", "v11", "v8"), RT_ASM_ARGS("s48", "s51", "s52", "s49", "s53", "s50", "s54", "s57", "s58", "s55", "s59", "s56")) \
    RT_ASM_CASE(7, RT_ASM_ARGS("v3", "v0", "v4", "v1", "v5", "v2", "v9", "v6", "v10", "v7", "v11", "v8"), RT_ASM_ARGS("s51", "s48", "s52", "s49", "s53", "s50", "s57", "s54", "s58", "s55", "s59", "s56"))
    // (the same eight loops with the ray's world origin in vector registers, and the any-hit form: the ray queries)
    if constexpr (ORGV) {
#define RT_ASM_ORG_C "v"
#define RT_ASM_CASE_ANYHIT(VN, SN) else if constexpr (ANYHIT) { RT_ASM_VARIANT(RT_ASM_NOCOUNT, RT_ASM_POPS_INTERIOR, RT_ASM_POPS_LEAF RT_ASM_ANYHIT_CLEAR, RT_ASM_ANYHIT_MARK, RT_ASM_ANYHIT_LEAVE, RT_ASM_OUT_ANYHIT, RT_ASM_ARGS(VN), RT_ASM_ARGS(SN)); }
        RT_ASM_ALL_CASES
#undef RT_ASM_ORG_C
#undef RT_ASM_CASE_ANYHIT
    } else {
#define RT_ASM_ORG_C "s"
#define RT_ASM_CASE_ANYHIT(VN, SN)
        RT_ASM_ALL_CASES
#undef RT_ASM_ORG_C
#undef RT_ASM_CASE_ANYHIT
    }
#undef RT_ASM_ALL_CASES
#undef RT_ASM_CASE
#undef RT_ASM_VARIANT
#undef RT_ASM_ARGS
#undef RT_ASM_COUNT
#undef RT_ASM_NOCOUNT
#undef RT_ASM_GO
#undef RT_ASM_GO2
#undef RT_ASM_OUT_PLAIN
#undef RT_ASM_OUT_POPS
#undef RT_ASM_OUT_LOC
#undef RT_ASM_OUT_ANYHIT
#undef RT_ASM_STACK_OUT
#undef RT_ASM_STACK_IN
    sp = (int32_t)(sa - column) >> (ROW_SHIFT - 2);
}

// Octant-specialised loops.  The rays of a wave -- an 8x8-pixel
// tile, or the samples of a few pixels -- almost always share the sign octant of their mesh-space direction: one ballot per
// instance decides whether the wave runs the loop instantiated for that octant (slab_oct: the min / max pairs of the slab test
// become operand choices) or the generic loop.  A wave qualifies when every active lane has a finite origin and finite,
// non-zero direction inverses of the same signs, and the mesh has no interior record with an unordered or NaN box
// (mesh_flags bit 0, kept by every writer of interior records: upload, device rebuild, refit).
// OCTANTS = false keeps one loop: the bounce / shadow kernels of the extension renderer carry their path state across every
// cast in registers they do not have (spilled to scratch); nine loops per cast site made that worse (c3 24.9 ms against
// 23.7 ms with the generic loop alone, profiles/r04_experiments/octants_in_extension_kernels.log), while the samples-only
// kernel, which carries nothing, gains like the primary kernel (c4 at 16 spp: 8.27 against 8.50 ms).
// VIEW: `view_off` = byte offset of the frame's view records from p.records (see trace_loop).
// UNIFORM_ORG: every lane's ray starts at the same point (primary rays; the hand-written loop takes the origin as scalars).
// STATS (rt_scene_loop_stats: an instrumented copy of the production kernels, never a timed launch): which loop this wave ran for
// this instance goes to p.loop_stats (RT_LOOP_*), one count per wave and instance.
__device__ __forceinline__ void loop_stat(const RenderParams& p, int which, unsigned long long n = 1ull)
{
    const unsigned long long active = __ballot(true);
    if ((int)(__lane_id()) == __ffsll((long long)active) - 1) atomicAdd(&p.loop_stats[which], n);
}

template <bool DEBUG, bool PROF, bool EX = false, bool COUNT = false, class STK = Stack, bool POPS = false, bool OCTANTS = true, bool ANYHIT = false,
          bool VIEW = false, bool UNIFORM_ORG = !EX, bool STATS = false, bool SEC = false, bool HDR = false>
__device__ __forceinline__ void trace_instance(const RenderParams& p, const DevInstance& in, int inst_index,
                                               V3 org, V3 dir, STK& stack, Hit& hit, Counters<DEBUG>& cnt, int* iters = nullptr,
                                               int* pops = nullptr, uint32_t view_off = 0, float tmax = FLT_MAX)
{
    // HDR (render_kernel<.., VIEW>): everything of the instance that is the same in every lane -- the origin in mesh space and whether
    // it is finite, the mesh's flags, the root, the view delta -- comes from the (frame, instance) ray header the view pre-pass wrote, in
    // one fetch through the scalar cache; the lane transforms its direction, with to_mesh_space's operations in their order.
    static_assert(!HDR || (VIEW && UNIFORM_ORG && OCTANTS && !EX && !SEC && !PROF && !DEBUG), "ray headers: the timed primary kernels' view path");
    const RayHeaderWords h = HDR ? ray_header(p, view_off, inst_index) : RayHeaderWords();
    const MeshRay r = HDR ? to_mesh_space(h, dir) : to_mesh_space(in, org, dir);
    const uint32_t vdelta = HDR ? h.vdelta : VIEW ? view_off + (uint32_t)p.view_inst_off[inst_index] : 0u;
    int oct = -1;
    if constexpr (!PROF && OCTANTS) {
        const float inf = __int_as_float(0x7f800000);
        const bool usable = fabsf(r.dinv.x) < inf && fabsf(r.dinv.y) < inf && fabsf(r.dinv.z) < inf &&
                            r.dinv.x != 0.0f && r.dinv.y != 0.0f && r.dinv.z != 0.0f &&
                            (HDR || (fabsf(r.ro.x) < inf && fabsf(r.ro.y) < inf && fabsf(r.ro.z) < inf));    // (HDR: kRayOriginFinite)
        const int mine = (r.dinv.x < 0.0f ? 1 : 0) | (r.dinv.y < 0.0f ? 2 : 0) | (r.dinv.z < 0.0f ? 4 : 0);
        const int first = __builtin_amdgcn_readfirstlane(mine);
        if ((HDR ? (h.flags & (kRayOriginFinite | kRayBoxUnordered)) == kRayOriginFinite : (p.mesh_flags[in.mesh_index] & 1) == 0) &&
            __ballot(!usable || mine != first) == 0ull) oct = first;
    }
    // SEC (round 6: a ray with an origin of its own per lane -- the ray queries' rays; an any-hit ray is done at its first hit -- on the
    // optimistic stack): the hand-written loop or nothing.  A wave it does not cover (mixed sign octants, an exact-uv mesh) leaves with sp != 0,
    // which is what an outgrown stack looks like: cast_ray_ex then casts the ray again on the general stack and the compiler's loop, so
    // a cast site holds the eight hand-written loops and ONE compiled loop.
    static_assert(!SEC || (OCTANTS && POPS && !VIEW && !UNIFORM_ORG && !STK::kSpill && !DEBUG && !PROF && !COUNT), "SEC");
    if constexpr (SEC) { if (!(oct >= 0 && in.exact_uv == 0)) { stack.sp = 1; return; } }
    if constexpr (OCTANTS && !DEBUG && !PROF && (UNIFORM_ORG || SEC) && (!EX || POPS) && !(POPS && COUNT) && (!ANYHIT || SEC) && !STK::kSpill) {
        // the hand-written loop (trace_loop_asm) for what it covers; everything else takes the C++ loops below
        if (SEC || (oct >= 0 && (HDR ? (h.flags & kRayExactUv) == 0 : in.exact_uv == 0))) {
            if constexpr (STATS) { loop_stat(p, RT_LOOP_ASM); if (HDR ? (h.flags & kRayUnitInv) == 0 : in.unit_inv == 0) loop_stat(p, RT_LOOP_ASM_POSED); }
            stack.sp = 0;
            stack.push(kSentinel);
            int32_t cur = HDR ? h.root_ref : in.root_ref, sp = stack.sp;
            int wave_iters = 0;
            static_assert(STK::kStride == 64 || STK::kStride == 256, "the stack column's row pitch as a shift");
            int no_pops = 0;
            // EX (the bounce kernel's primary ray keeps the hit's world location): the loop hands back the accepted candidate's point in
            // mesh space; whether it accepted anything shows in the instance field, which it overwrites
            V3 point = v3(0.0f, 0.0f, 0.0f);
            const int32_t instance_before = hit.instance;
            if constexpr (EX) hit.instance = -7;
            // (wave-uniform values read through the scalar cache: the instance record's address is uniform)
            const V3 back = HDR ? h.back : v3(in.inv_pose_xyz[0], in.inv_pose_xyz[1], in.inv_pose_xyz[2]);
            const uintptr_t ia = (HDR ? (h.flags & kRayUnitInv) != 0 : in.unit_inv != 0) ? (uintptr_t)0 : (uintptr_t)&in;
            const DevInstance* general = (const DevInstance*)(((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ia >> 32)) << 32) |
                                                              (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ia));
#define RT_TRACE_ASM(O) trace_loop_asm<O, COUNT, (STK::kStride == 64 ? 8 : 10), VIEW, POPS, EX, SEC, ANYHIT>(p, inst_index, r, org, stack.lds, stack.lds_depth, cur, sp, hit, wave_iters, vdelta, \
                                                                                              POPS ? *pops : no_pops, point, back, general, tmax)
            switch (oct) {
            case 0: RT_TRACE_ASM(0); break;
            case 1: RT_TRACE_ASM(1); break;
            case 2: RT_TRACE_ASM(2); break;
            case 3: RT_TRACE_ASM(3); break;
            case 4: RT_TRACE_ASM(4); break;
            case 5: RT_TRACE_ASM(5); break;
            case 6: RT_TRACE_ASM(6); break;
            default: RT_TRACE_ASM(7); break;
            }
#undef RT_TRACE_ASM
            stack.sp = sp;
            if constexpr (COUNT) *iters += wave_iters;          // (the wave's iterations = those of its longest lane, which is what the tile cost is)
            if constexpr (EX) {
                if (hit.instance == -7) hit.instance = instance_before;
                else {                                          // raycast.cu:98-104, as triangle_test<.., EX> does it for every candidate
                    V3 loc = v3(point.x * in.scale[0], point.y * in.scale[1], point.z * in.scale[2]);
                    hit.loc = apply_quat(in.q_inv_pose, v3(loc.x - in.inv_pose_xyz[0], loc.y - in.inv_pose_xyz[1], loc.z - in.inv_pose_xyz[2]));
                }
            }
            return;
        }
    }
    if constexpr (SEC) return;                                  // (never reached: both ways out are above)
    else {
    // (the C++ loop reads view records for the primary kernels' rays only; an extension ray that does not qualify for the hand-written
    // loop reads the records themselves)
    // (STATS: the lanes' iterations on the compiler's loops are counted too, RT_LOOP_CPP_ITERS -- the loops that take a view's box
    // words through the generic slab test)
    static_assert(!(STATS && COUNT), "one iteration counter");
    int stat_iters = 0;
#define RT_TRACE_LOOP(O) trace_loop<DEBUG, PROF, EX, (COUNT || STATS), STK, POPS, O, ANYHIT, (VIEW && !EX)>(p, in, inst_index, r, org, stack, hit, cnt, STATS ? &stat_iters : iters, pops, vdelta, tmax)
    if constexpr (STATS) loop_stat(p, STK::kSpill ? RT_LOOP_DEEP : (oct >= 0 ? RT_LOOP_CPP_OCTANT : RT_LOOP_CPP_GENERIC));
    switch (oct) {                                              // (wave-uniform: a scalar branch)
    case 0: RT_TRACE_LOOP(0); break;
    case 1: RT_TRACE_LOOP(1); break;
    case 2: RT_TRACE_LOOP(2); break;
    case 3: RT_TRACE_LOOP(3); break;
    case 4: RT_TRACE_LOOP(4); break;
    case 5: RT_TRACE_LOOP(5); break;
    case 6: RT_TRACE_LOOP(6); break;
    case 7: RT_TRACE_LOOP(7); break;
    default: RT_TRACE_LOOP(-1); break;
    }
#undef RT_TRACE_LOOP
    if constexpr (STATS) atomicAdd(&p.loop_stats[RT_LOOP_CPP_ITERS], (unsigned long long)stat_iters);
    }
}

__device__ __forceinline__ uint8_t to_u8(float f) { return (uint8_t)(int)f; }

// texture / albedo colour of a hit, raycast.cu:224-245 (ray.color starts at 1,1,1: Ray.hpp:22)
__device__ __forceinline__ V3 base_colour(const RenderParams& p, const Hit& hit)
{
    const DevInstance& in = p.instances[hit.instance];
    const DevMaterial& m = p.materials[in.material_index];
    if (m.texture_width > 0) {                                  // raycast.cu:224-240
        float2 uv = make_float2(hit.u, hit.v);                  // exact-uv meshes: the hit carries uv itself
        if (!in.exact_uv) {
            const float* q = p.tri_uv + (size_t)hit.slot * 6;
            float w = 1.0f - hit.u - hit.v;
            uv.x = (w * q[0] + hit.v * q[2]) + hit.u * q[4];
            uv.y = (w * q[1] + hit.v * q[3]) + hit.u * q[5];
        }
        int tex_x = (int)(uv.x * (float)m.texture_width);
        int tex_y = (int)((1.0 - (double)uv.y) * (double)(float)m.texture_height);
        tex_x = (int)fmaxf((float)(tex_x % m.texture_width), 0.0f);
        tex_y = (int)fmaxf((float)(tex_y % m.texture_height), 0.0f);
        const uint8_t* tc = m.texture + (size_t)tex_y * m.texture_pitch + 3 * (size_t)tex_x;
        return v3(1.0f * ((float)tc[0] * 0.0039215f), 1.0f * ((float)tc[1] * 0.0039215f), 1.0f * ((float)tc[2] * 0.0039215f));
    }
    return v3(1.0f * m.albedo[0], 1.0f * m.albedo[1], 1.0f * m.albedo[2]);     // raycast.cu:241-245
}

// raycast.cu:207-294 -> the pixel's three bytes packed as x | y << 8 | z << 16
__device__ __forceinline__ uint32_t shade(const RenderParams& p, const Hit& hit)
{
    if (hit.min == FLT_MAX) return 255u | (204u << 8) | (153u << 16);      // sky, raycast.cu:208-216
    const V3 c = base_colour(p, hit);
    const float illumination = 1.0f;                            // raycast.cu:282-290
    return (uint32_t)to_u8(illumination * c.x * 255.0f) |       // raycast.cu:292-294
           ((uint32_t)to_u8(illumination * c.y * 255.0f) << 8) |
           ((uint32_t)to_u8(illumination * c.z * 255.0f) << 16);
}

// pixel of thread `tid` in the 16x16 tile at (x0, y0): a wave64 is an 8x8-pixel block (neighbouring rays walk the same nodes:
// L1 hits, little divergence).  (x, ly) = column and LOCAL row; y = frame row (they differ only when rendering stripes).
__device__ __forceinline__ void pixel_of(const RenderParams& p, const FrameParams& f, int tid, int x0, int y0, int& x, int& ly, int& y)
{
    const int wave = tid >> 6, lane = tid & 63;
    // (rows of eight lanes; Z-order inside the 8x8 block made no difference on any camera: profiles/r04_experiments/sentinel_loop_ab.log)
    const int lx = lane & 7, lyy = lane >> 3;
    x = x0 + (wave & 1) * 8 + lx;
    ly = y0 + (wave >> 1) * 8 + lyy;
    y = ly;                                                     // stripes: local row -> frame row (the identity for one rank)
    if (p.num_ranks != 1) y = ((ly / p.stripe_rows) * p.num_ranks + f.rank) * p.stripe_rows + ly % p.stripe_rows;
}

// whether render_kernel<DEBUG, PROF, ., SPILL> runs the optimistic stack (StackT), and the rows of its LDS block
template <bool DEBUG, bool PROF, bool SPILL>
__host__ __device__ constexpr bool optimistic_stack() { return SPILL && !DEBUG && !PROF; }
template <bool DEBUG, bool PROF, bool SPILL>
__host__ __device__ inline int lds_block_rows(int stack_depth) { return lds_rows(stack_depth) + (optimistic_stack<DEBUG, PROF, SPILL>() ? 1 : 0); }

// One pixel: camera ray -> cast_ray over all instances -> flat shade -> store (raycast.cu:146-297).
// TABLE (with VIEW, the un-ordered grid, one rank): the lane's camera-space direction comes from the launch's direction table --
// three coalesced 256-byte loads per wave, issued before anything else so that the ray header's scalar fetch runs beside them --
// and holds the bits camera_space_direction would have computed here: the pre-pass wrote them with that function.
// GBUF (rt_render_gbuffer, gbuffer_kernel below): the traversal is the one of the timed kernels, untouched; the epilogue also stores the
// G-buffer planes of `g`, frame-major (frame = blockIdx.z of the un-ordered grid), and shades only a frame that has an image.  The
// planes beyond t and the ids are derived AFTER the traversal from what it leaves (hit.instance, hit.slot, hit.u, hit.v) and the
// pixel's ray made again: the loop keeps no location -- three more live registers there cost every ray, the second evaluation of one
// triangle costs a hit pixel a few dozen instructions once.
struct GBufParams {
    float* t;                   // every plane optional (null = not wanted), tight, [frame][height][width](xk): RtGBuffer of rt_hip.h
    float* depth;
    int32_t *instance, *triangle;
    float *location, *normal, *uv;
    Q4 q_pose[kMaxBatch];       // euler2quat(camera_pose ypr) of frame i: the rotation of apply_lre(camera_pose, .), for `depth`
};
static_assert(sizeof(RenderParams) + sizeof(GBufParams) <= 4096, "kernel arguments must fit in 4 KB");
__device__ __forceinline__ V3 hit_normal(const RenderParams& p, const Hit& hit);

// ROLL (rt_render_gbuffer_rolling, rolling_gbuffer_kernel below): the pose of one slice of one rolling frame, packed by the host -- the
// quaternions are the host's euler2quat, so their bits are those of rt_ray_table_rays and GBufParams::q_pose.  One record per frame
// and slice, [frame][slice], in the caller's workspace; a wave reads its own with scalar loads (the address space says the words do
// not change while the kernel runs: the records were written earlier in the stream's order).
struct RollRecord {
    float origin[3];            // camera_pose xyz of the slice, as FrameParams::origin
    uint32_t pad;
    Q4 q_cam;                   // euler2quat(inv_camera_pose ypr), as FrameParams::q_cam
    Q4 q_pose;                  // euler2quat(camera_pose ypr), as GBufParams::q_pose
};
static_assert(sizeof(RollRecord) == 48, "three scalar fetches of four words");
typedef const __attribute__((address_space(4))) RollRecord* RollRecordPtr;
struct RollParams {
    const RollRecord* records;  // [num_frames][slices]
    float* local;               // optional plane [frame][height][width][3]: apply_lre(camera_pose of the pixel's slice, location)
    int32_t slices;
    int32_t axis;               // 0: the column x selects the slice, 1: the row y
    int32_t slice_tiles;        // slice_pixels / 8: a slice is whole tiles
};
static_assert(sizeof(RenderParams) + sizeof(GBufParams) + sizeof(RollParams) <= 4096, "kernel arguments must fit in 4 KB");

template <bool DEBUG, bool PROF, bool COUNT = false, bool SPILL = true, bool VIEW = false, bool STATS = false, bool TABLE = false, bool GBUF = false, bool ROLL = false>
__device__ __forceinline__ void render_pixel(const RenderParams& p, const FrameParams& f, int x0, int y0, lds_int* lds_base, lds_int*& lds_column,
                                             int* iters = nullptr, uint32_t view_off = 0, const GBufParams* g = nullptr,
                                             const Q4* roll_q_pose = nullptr, float* roll_local = nullptr)
{
    // (a caller's table -- RtRayTable, rt_render_gbuffer_table -- also serves a launch without view records: the G-buffer form only)
    static_assert(!TABLE || ((VIEW || GBUF) && !COUNT && !DEBUG && !PROF && kPrimBlock == 64), "direction table: the batched view kernels and the G-buffer kernels, one 8x8 tile per workgroup");
    static_assert(!GBUF || (!COUNT && !DEBUG && !PROF && !STATS && kPrimBlock == 64), "G-buffer: the un-ordered production kernels");
    // (f is then the kernel's own copy: origin and q_cam from the slice's record, img / rank / local_rows from p.frames[frame])
    static_assert(!ROLL || (GBUF && TABLE && !VIEW), "rolling frames: the caller's table over plain records");
    V3 cdir;
    if constexpr (TABLE) {
        const float* t = p.dir_table + ((size_t)(blockIdx.y * (unsigned)p.tiles_x + blockIdx.x) * (3 * 64) + (size_t)(lds_column - lds_base));
        cdir = v3(t[0], t[64], t[128]);
    }
    int x, ly, y;
    pixel_of(p, f, (int)(lds_column - lds_base), x0, y0, x, ly, y);
    const V3 org = v3(f.origin[0], f.origin[1], f.origin[2]);
    if constexpr (!TABLE) cdir = camera_space_direction(f, (float)x, (float)y);
    const V3 dir = world_direction(f, cdir);

    Hit hit;
    hit.min = FLT_MAX; hit.slot = -1; hit.instance = -1; hit.u = 0.0f; hit.v = 0.0f;
    Counters<DEBUG> cnt;
    if constexpr (optimistic_stack<DEBUG, PROF, SPILL>()) {
        // A tree deeper than the LDS part of the stack, a ray that (almost always) is not: the LDS-only loops, and the general
        // stack only for the lanes that turn out to need it -- from the start of the ray, so the hit is the one the general kernel
        // finds (the instrumented kernel keeps the general stack throughout: its counts are per ray, not per attempt).
        StackT<kPrimBlock, false, true> stack;
        stack.lds = lds_column; stack.spill = nullptr; stack.lds_depth = lds_rows(p.stack_depth); stack.sp = 0;
        int outgrown = 0;                                       // a loop left through the spare row ends with sp != 0
        for (int i = 0; i < p.num_instances; i++) {             // raycast.cu:26
            trace_instance<DEBUG, PROF, false, COUNT, StackT<kPrimBlock, false, true>, false, true, false, VIEW, true, STATS, false, VIEW>(p, p.instances[i], i, org, dir, stack, hit, cnt,
                                                                                                                         iters, nullptr, view_off);
            outgrown |= stack.sp;
        }
        if constexpr (STATS) { loop_stat(p, RT_LOOP_WAVES); if (__ballot(outgrown != 0) != 0ull) loop_stat(p, RT_LOOP_RETRACED_LANES, (unsigned long long)__popcll(__ballot(outgrown != 0))); }
        if (outgrown != 0) {
            int spill[kMaxStack - kLdsStack];
            StackT<kPrimBlock, true> deep;
            deep.lds = lds_column; deep.spill = spill; deep.lds_depth = lds_rows(p.stack_depth); deep.sp = 0;
            hit.min = FLT_MAX; hit.slot = -1; hit.instance = -1; hit.u = 0.0f; hit.v = 0.0f;
            for (int i = 0; i < p.num_instances; i++)
                trace_instance<DEBUG, PROF, false, COUNT, StackT<kPrimBlock, true>, false, false, false, false, true, STATS>(p, p.instances[i], i, org, dir, deep, hit, cnt, iters);
        }
    } else {
        int spill[SPILL ? kMaxStack - kLdsStack : 1];
        StackT<kPrimBlock, SPILL> stack;
        stack.lds = lds_column; stack.spill = spill; stack.lds_depth = lds_rows(p.stack_depth); stack.sp = 0;
        if constexpr (STATS) loop_stat(p, RT_LOOP_WAVES);
        for (int i = 0; i < p.num_instances; i++)               // raycast.cu:26
            trace_instance<DEBUG, PROF, false, COUNT, StackT<kPrimBlock, SPILL>, false, true, false, VIEW, true, STATS, false, VIEW>(p, p.instances[i], i, org, dir, stack, hit, cnt, iters,
                                                                                                               nullptr, view_off);
    }

    // The pixel's coordinates are not kept across the traversal (three registers in a kernel that has none to spare: they
    // were spilled to scratch): they are derived again from the one per-thread value the loop keeps anyway, the address of
    // the lane's LDS stack column.  (The empty asm hides that address's origin from the optimiser, which would otherwise
    // recognise the recomputation and keep the first copies alive.)
    asm volatile("" : "+v"(lds_column));
    pixel_of(p, f, (int)(lds_column - lds_base), x0, y0, x, ly, y);
    if (!GBUF || f.img) {                                       // (G-buffer frames without an image: no texture fetch, no store)
        const uint32_t px = shade(p, hit);
        uint8_t* out = f.img + (size_t)ly * p.pitch + 3 * (size_t)x;
        out[0] = (uint8_t)px; out[1] = (uint8_t)(px >> 8); out[2] = (uint8_t)(px >> 16);
    }
    if constexpr (GBUF) {
        // element of pixel (x, y) of this frame in a scalar plane; every offset in size_t
        const size_t o = ((size_t)blockIdx.z * (size_t)p.height + (size_t)y) * (size_t)p.width + (size_t)x;
        const bool got = hit.instance >= 0;
        if (g->t) g->t[o] = hit.min;
        if (g->instance) g->instance[o] = hit.instance;
        if (g->triangle) g->triangle[o] = got ? p.tri_id[hit.slot] : -1;
        bool want_local = false;
        if constexpr (ROLL) want_local = roll_local != nullptr;
        if (g->location || g->depth || want_local) {
            // The accepted candidate once more, as triangle_test<.., EX> evaluates it for query_kernel (raycast.cu:33-51, TrianglePrimitive.hpp:62-79,
            // raycast.cu:98-104): the pixel's ray from the same table entry or the same intrinsics, to_mesh_space of the winning
            // instance, the record of the winning slot, the transform always applied.  Same operations on the same inputs: the
            // bits of rt_trace_rays' location.
            V3 loc = v3(0.0f, 0.0f, 0.0f);
            float depth = FLT_MAX;
            V3 local = v3(0.0f, 0.0f, 0.0f);                    // (ROLL only)
            if (got) {
                V3 cd;
                if constexpr (TABLE) {
                    const float* t = p.dir_table + ((size_t)(blockIdx.y * (unsigned)p.tiles_x + blockIdx.x) * (3 * 64) + (size_t)(lds_column - lds_base));
                    cd = v3(t[0], t[64], t[128]);
                } else cd = camera_space_direction(f, (float)x, (float)y);
                const V3 wd = world_direction(f, cd);
                const V3 o3 = v3(f.origin[0], f.origin[1], f.origin[2]);
                const DevInstance& in = p.instances[hit.instance];
                const MeshRay r = to_mesh_space(in, o3, wd);
                const float4* rec = p.records + (size_t)hit.slot * 4;
                const float4 t0 = rec[0], t1 = rec[1];
                const V3 v0 = v3(t0.x, t0.y, t0.z), nrm = v3(t0.w, t1.x, t1.y);
                const float denom = dot(r.rd, nrm);
                const float tt = dot(v0 - r.ro, nrm) / denom;
                const V3 pt = r.ro + tt * r.rd;
                loc = v3(pt.x * in.scale[0], pt.y * in.scale[1], pt.z * in.scale[2]);
                loc = apply_quat(in.q_inv_pose, v3(loc.x - in.inv_pose_xyz[0], loc.y - in.inv_pose_xyz[1], loc.z - in.inv_pose_xyz[2]));
                // depth (rt_hip.h, G-buffer rule 2): apply_lre(camera_pose, location).z
                if constexpr (ROLL) {
                    // rolling frames rule 2: all three components of apply_lre(camera_pose of the slice, location); depth is its z
                    local = apply_quat(*roll_q_pose, v3(loc.x - f.origin[0], loc.y - f.origin[1], loc.z - f.origin[2]));
                    depth = local.z;
                } else
                depth = apply_quat(g->q_pose[blockIdx.z], v3(loc.x - f.origin[0], loc.y - f.origin[1], loc.z - f.origin[2])).z;
            }
            if (g->location) { g->location[o * 3] = loc.x; g->location[o * 3 + 1] = loc.y; g->location[o * 3 + 2] = loc.z; }
            if (g->depth) g->depth[o] = depth;
            if constexpr (ROLL) if (want_local) { roll_local[o * 3] = local.x; roll_local[o * 3 + 1] = local.y; roll_local[o * 3 + 2] = local.z; }
        }
        if (g->normal) {
            const V3 n = got ? hit_normal(p, hit) : v3(0.0f, 0.0f, 0.0f);
            g->normal[o * 3] = n.x; g->normal[o * 3 + 1] = n.y; g->normal[o * 3 + 2] = n.z;
        }
        if (g->uv) {
            // query_kernel's uv: TrianglePrimitive::point_inside's interpolation (exact-uv meshes: the hit carries it)
            float2 uv = make_float2(0.0f, 0.0f);
            if (got) {
                uv = make_float2(hit.u, hit.v);
                if (!p.instances[hit.instance].exact_uv) {
                    const float* q = p.tri_uv + (size_t)hit.slot * 6;
                    const float w = 1.0f - hit.u - hit.v;
                    uv.x = (w * q[0] + hit.v * q[2]) + hit.u * q[4];
                    uv.y = (w * q[1] + hit.v * q[3]) + hit.u * q[5];
                }
            }
            g->uv[o * 2] = uv.x; g->uv[o * 2 + 1] = uv.y;
        }
    }

    // hit-id planes: also available from the production kernel (rt_render_ids), so that the kernel that is timed is the
    // kernel whose hit ids are checked; a wave-uniform branch on a kernel argument, outside the traversal loop
    if (p.hit_instance || p.hit_triangle) {
        const size_t o = (size_t)y * p.width + x;
        if (p.hit_instance) p.hit_instance[o] = hit.instance;
        if (p.hit_triangle) p.hit_triangle[o] = hit.slot >= 0 ? p.tri_id[hit.slot] : -1;
    }
    if constexpr (DEBUG) {
        size_t o = (size_t)y * p.width + x;
        if (p.node_pops) p.node_pops[o] = cnt.pops;
        if (p.aabb_tests) p.aabb_tests[o] = cnt.aabb;
        if (p.tri_tests) p.tri_tests[o] = cnt.tris;
        if (p.inside_hits) p.inside_hits[o] = cnt.inside;
    }
}

// ORDERED (single-frame launches, see launch()): workgroup b renders tile tile_order[b] --
// the tiles that took longest in the previous frame first -- and the last wave of every workgroup to finish records the workgroup's cost for the
// next frame's order (cost = loop iterations of its longest lane).  A frame rendered alone ends in a tail of a few long waves (rays grazing the silhouette) on an
// otherwise idle chip; started first, those waves run beside the bulk of the frame instead of after it
// (measured: -22 % / -12 % / 0 % frame time for the far / mid / near camera).  Which tile a workgroup renders does not
// change what a pixel computes.
template <bool DEBUG, bool PROF, bool ORDERED = false, bool SPILL = true, bool VIEW = false, bool STATS = false, bool TABLE = false>
__global__ __launch_bounds__(kPrimBlock, 8) void render_kernel(const RenderParams p)
{
    static_assert(!TABLE || (VIEW && !ORDERED), "direction table: its tile index is the un-ordered grid's");
    extern __shared__ int lds_stack[];                          // [lds_block_rows(stack_depth)][kPrimBlock] (+ 2 ints when ORDERED)

    // Workgroup (x, y) of frame z renders tile (x, y): row-major, as workgroups are dispatched -- the tile's coordinates need no
    // division.  Consecutive workgroups are dealt round-robin to the 8 XCDs, so every
    // XCD sees tiles from the whole frame: measured faster than giving each XCD one contiguous band (better load
    // balance; the working set is L1/L2 resident either way).
    int tile = (int)blockIdx.x, frame = ORDERED ? 0 : (int)blockIdx.z;
    int iters = 0;
    if constexpr (ORDERED) {
        // a one-dimensional grid: workgroup b renders frame b % F of the tile with rank b / F, so the costly tiles of ALL
        // frames of a batch come first and the launch ends with cheap ones
        frame = tile % p.num_frames;
        tile = tile / p.num_frames;
        if (p.tile_order) tile = p.tile_order[tile];
    }
    const int tx = ORDERED ? tile % p.tiles_x : (int)blockIdx.x, ty = ORDERED ? tile / p.tiles_x : (int)blockIdx.y;

    unsigned long long t_start = 0;
    if (p.trace) t_start = wall_clock64();
    // the thread's index lives on as the address of its LDS stack column only (see render_pixel)
    lds_int* column = (lds_int*)lds_stack + threadIdx.x;
    {
        int x, ly, y;
        pixel_of(p, p.frames[frame], (int)threadIdx.x, tx * kPrimTile, ty * kPrimTile, x, ly, y);
        if (x < p.width && ly < p.frames[frame].local_rows)
            render_pixel<DEBUG, PROF, ORDERED, SPILL, VIEW, STATS, TABLE>(p, p.frames[frame], tx * kPrimTile, ty * kPrimTile, (lds_int*)lds_stack, column, &iters,
                                                            VIEW ? p.view_base + (uint32_t)frame * p.view_frame_stride : 0u);
    }
    asm volatile("" : "+v"(column));
    const int tid = (int)(column - (lds_int*)lds_stack), wave = tid >> 6, lane = tid & 63;
    if constexpr (ORDERED) {
        // cost of the tile = loop iterations of its longest lane: deterministic, unlike a lifetime, which also measures
        // how full the chip was while the workgroup ran
        static_assert(!ORDERED || kPrimBlock == 64, "one wave per workgroup: the wave's longest lane is the tile's");
        for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(iters, o); iters = v > iters ? v : iters; }
        // Round 6: the cost goes to the tile AND ITS EIGHT NEIGHBOURS, as a maximum (nine lanes, one atomic each; the sort clears what
        // it has read).  The costly tiles are the ones whose rays graze a silhouette, and which tiles those are changes with the
        // smallest camera motion: a frame a few millimetres along finds last frame's order one tile off exactly where it matters
        // (single frames along bench.py's 4 mm camera loop 0.134 ms, the same pose repeated 0.127: single_frame_gap.md).  With the
        // neighbourhood's maximum the tiles NEXT to a costly one start early too; several frames per launch (a rank's stripes of a
        // few frames, which differ in pose and, with a rotating owner, in the rows a tile stands for) add up the same way.
        if (p.tile_cost && lane < 9) {
            const int nx = tile % p.tiles_x + lane % 3 - 1, ny = tile / p.tiles_x + lane / 3 - 1;
            if (nx >= 0 && nx < p.tiles_x && ny >= 0 && ny < p.tiles_y) atomicMax(&p.tile_cost[ny * p.tiles_x + nx], iters);
        }
    }
    if (p.trace && lane == 0) {                                 // diagnostic: per-wave lifetime (RT_TRACE_FILE)
        // (the ordered grid is one-dimensional: its y and z are 0, and the two-term form keeps that kernel's code what it was)
        const size_t wg = ORDERED ? (size_t)blockIdx.y * gridDim.x + blockIdx.x : trace_workgroup();
        unsigned long long* t = p.trace + (wg * (kPrimBlock / 64) + wave) * 16;
        t[0] = t_start; t[1] = wall_clock64();
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        t[2] = ((unsigned long long)xcc << 32) | hw; t[3] = (unsigned long long)(ORDERED ? tile : (int)(blockIdx.y * gridDim.x + blockIdx.x));
    }
}

// rt_render_gbuffer: render_kernel's un-ordered form -- workgroup (x, y) of frame z renders tile (x, y), one wave per workgroup, the
// same LDS block -- around render_pixel<.., GBUF>, with the planes as a second kernel argument (as query_kernel takes QueryParams):
// a kernel of its own because the arguments of render_kernel's instantiations must stay what they are.  No heavy-first order, no
// wave stamps: neither applies to this call.  TABLE without VIEW: the table is the caller's (rt_render_gbuffer_table), the launch got
// no view slot.
template <bool SPILL, bool VIEW, bool TABLE>
__global__ __launch_bounds__(kPrimBlock, 8) void gbuffer_kernel(const RenderParams p, const GBufParams g)
{
    extern __shared__ int lds_stack[];                          // [lds_block_rows(stack_depth)][kPrimBlock]
    const int frame = (int)blockIdx.z, x0 = (int)blockIdx.x * kPrimTile, y0 = (int)blockIdx.y * kPrimTile;
    lds_int* column = (lds_int*)lds_stack + threadIdx.x;
    int x, ly, y;
    pixel_of(p, p.frames[frame], (int)threadIdx.x, x0, y0, x, ly, y);
    if (x < p.width && ly < p.frames[frame].local_rows)
        render_pixel<false, false, false, SPILL, VIEW, false, TABLE, true>(p, p.frames[frame], x0, y0, (lds_int*)lds_stack, column, nullptr,
                                                                           VIEW ? p.view_base + (uint32_t)frame * p.view_frame_stride : 0u, &g);
}

// rt_render_gbuffer_rolling (include/rt_hip.h "rolling frames"): gbuffer_kernel<SPILL, false, true> -- the
// caller's table over plain records, the same grid, LDS block and launch bounds -- with a pose per slice of whole tiles.  A workgroup
// is one wave and one tile, so the wave still has ONE origin and ONE rotation: its slice is an expression of blockIdx, hence provably
// wave-uniform, and the slice's record arrives by scalar loads into the kernel's own copy of the frame's parameters.  The traversal
// is the timed one, untouched; img, rank and local_rows are the frame's.  The slice index is bounded by `slices` before the record is
// read.
template <bool SPILL>
__global__ __launch_bounds__(kPrimBlock, 8) void rolling_gbuffer_kernel(const RenderParams p, const GBufParams g, const RollParams r)
{
    extern __shared__ int lds_stack[];                          // [lds_block_rows(stack_depth)][kPrimBlock]
    const int frame = (int)blockIdx.z, x0 = (int)blockIdx.x * kPrimTile, y0 = (int)blockIdx.y * kPrimTile;
    int slice = (int)(r.axis ? blockIdx.y : blockIdx.x) / r.slice_tiles;
    slice = slice < r.slices ? slice : r.slices - 1;
    const RollRecordPtr rec = (RollRecordPtr)(uintptr_t)(r.records + ((size_t)frame * (size_t)r.slices + (size_t)slice));
    FrameParams f;                                              // (kinv and D: not read under a table)
    f.origin[0] = rec->origin[0]; f.origin[1] = rec->origin[1]; f.origin[2] = rec->origin[2];
    f.q_cam.x = rec->q_cam.x; f.q_cam.y = rec->q_cam.y; f.q_cam.z = rec->q_cam.z; f.q_cam.w = rec->q_cam.w;
    f.img = p.frames[frame].img; f.rank = p.frames[frame].rank; f.local_rows = p.frames[frame].local_rows;
    Q4 q_pose;
    q_pose.x = rec->q_pose.x; q_pose.y = rec->q_pose.y; q_pose.z = rec->q_pose.z; q_pose.w = rec->q_pose.w;
    lds_int* column = (lds_int*)lds_stack + threadIdx.x;
    int x, ly, y;
    pixel_of(p, f, (int)threadIdx.x, x0, y0, x, ly, y);
    if (x < p.width && ly < f.local_rows)
        render_pixel<false, false, false, SPILL, false, false, true, true, true>(p, f, x0, y0, (lds_int*)lds_stack, column, nullptr, 0u, &g, &q_pose, r.local);
}

// Point clouds (rt_point_cloud_offsets / rt_point_cloud_fill, include/rt_hip.h "point clouds"): the kept pixels
// of the staged G-buffer planes, packed in (frame, y, x) order.  A chunk is 64 consecutive pixels of ONE frame's row-major order -- a
// frame has chunks_per_frame = ceil(px / 64) of them, the last one partial -- and one wave works on one chunk: its 64-bit ballot of the
// keep predicate is the chunk's count (popcount) and every kept lane's place in the chunk (mbcnt).  No atomics and no dependence on
// the order of workgroups: the order of the points is the order of the pixels.  Four chunks per workgroup of 256 threads.
constexpr int kCloudBlock = 256, kCloudChunk = 64;
struct CloudCountParams {
    const float* t;             // staged planes [count][px]
    const int32_t* instance;
    const uint8_t* mask;        // [px] or null
    int64_t px;                 // pixels per frame
    int32_t chunks_per_frame, nchunks;
    float min_range, max_range;
    int32_t* counts;            // [nchunks]: what the scan reads
    unsigned long long* keep;   // [nchunks]: the chunk's ballot, for the fill (which is given neither the gate nor the mask)
};
__global__ __launch_bounds__(kCloudBlock) void cloud_count_kernel(const CloudCountParams c)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t chunk = (int64_t)blockIdx.x * (kCloudBlock / kCloudChunk) + ((int)threadIdx.x >> 6);
    if (chunk >= (int64_t)c.nchunks) return;                    // (wave-uniform)
    const int32_t frame = (int32_t)chunk / c.chunks_per_frame;
    const int64_t at = (int64_t)((int32_t)chunk - frame * c.chunks_per_frame) * kCloudChunk + lane;     // pixel y * width + x
    bool keep = false;
    if (at < c.px) {
        const size_t o = (size_t)frame * (size_t)c.px + (size_t)at;
        const float t = c.t[o];
        keep = c.instance[o] >= 0 && t >= c.min_range && t <= c.max_range && (!c.mask || c.mask[at] != 0);
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) { c.counts[chunk] = __popcll(b); c.keep[chunk] = b; }
}

// d_offsets[i] = the scanned offset of frame i's first chunk; d_offsets[count] = the total
__global__ __launch_bounds__(64) void cloud_frame_offsets_kernel(const int64_t* chunk_offsets, int32_t chunks_per_frame, int32_t count, int64_t* d_offsets)
{
    const int i = (int)threadIdx.x;
    if (i <= count) d_offsets[i] = chunk_offsets[(size_t)i * (size_t)chunks_per_frame];
}

struct CloudFillParams {
    const int64_t* chunk_offsets;       // [nchunks + 1], scanned
    const unsigned long long* keep;     // [nchunks]
    const float* t;                     // staged planes; those the fields did not stage are null and their outputs are too
    const int32_t *instance, *triangle;
    const float *location, *normal, *uv;
    int64_t px;
    int32_t chunks_per_frame, nchunks;
    int64_t capacity;
    float* range;                       // RtPointCloud
    int32_t *pixel, *frame, *out_instance, *out_triangle;
    float *position, *local, *out_normal, *out_uv;
    Q4 q_pose[kMaxBatch];               // euler2quat(camera_pose ypr) of frame i, as GBufParams::q_pose
    float origin[kMaxBatch][3];         // camera_pose xyz of frame i, as FrameParams::origin
};
static_assert(sizeof(CloudFillParams) <= 4096, "kernel arguments must fit in 4 KB");
// Everything read from the workspace is data: the pixel index is bounded by px before any plane is read and the slot -- compared as an
// unsigned number, so that a negative offset of a stale workspace is large -- by capacity before anything is written.
// ROLL (rt_point_cloud_fill_rolling): `local` takes the pose of the point's slice from the records rt_point_cloud_offsets_rolling left
// in the workspace -- data like the rest: the slice index is bounded by `slices` before a record is read.  q_pose and origin of `c`
// are then not read.
struct CloudRollParams {
    const RollRecord* records;  // [count][slices]
    int32_t width, slices, axis, slice_pixels;
};
__global__ __launch_bounds__(kCloudBlock) void cloud_fill_kernel(const CloudFillParams c)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t chunk = (int64_t)blockIdx.x * (kCloudBlock / kCloudChunk) + ((int)threadIdx.x >> 6);
    if (chunk >= (int64_t)c.nchunks) return;                    // (wave-uniform)
    const int32_t frame = (int32_t)chunk / c.chunks_per_frame;
    const int64_t at = (int64_t)((int32_t)chunk - frame * c.chunks_per_frame) * kCloudChunk + lane;
    const unsigned long long b = c.keep[chunk];                 // the count kernel's ballot
    if (at >= c.px || !((b >> lane) & 1ull)) return;
    // kept lanes below this one: v_mbcnt_lo / v_mbcnt_hi of the ballot
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    const unsigned long long slot = (unsigned long long)c.chunk_offsets[chunk] + below;
    if (slot >= (unsigned long long)c.capacity) return;
    const size_t o = (size_t)frame * (size_t)c.px + (size_t)at, j = (size_t)slot;
    if (c.range) c.range[j] = c.t[o];
    if (c.pixel) c.pixel[j] = (int32_t)at;
    if (c.frame) c.frame[j] = frame;
    if (c.out_instance) c.out_instance[j] = c.instance[o];
    if (c.out_triangle) c.out_triangle[j] = c.triangle[o];
    if (c.position || c.local) {
        const V3 loc = v3(c.location[o * 3], c.location[o * 3 + 1], c.location[o * 3 + 2]);
        if (c.position) { c.position[j * 3] = loc.x; c.position[j * 3 + 1] = loc.y; c.position[j * 3 + 2] = loc.z; }
        if (c.local) {
            // rt_hip.h, point clouds rule 5: render_pixel's depth expression, all three components
            const V3 l = apply_quat(c.q_pose[frame], v3(loc.x - c.origin[frame][0], loc.y - c.origin[frame][1], loc.z - c.origin[frame][2]));
            c.local[j * 3] = l.x; c.local[j * 3 + 1] = l.y; c.local[j * 3 + 2] = l.z;
        }
    }
    if (c.out_normal) { c.out_normal[j * 3] = c.normal[o * 3]; c.out_normal[j * 3 + 1] = c.normal[o * 3 + 1]; c.out_normal[j * 3 + 2] = c.normal[o * 3 + 2]; }
    if (c.out_uv) { c.out_uv[j * 2] = c.uv[o * 2]; c.out_uv[j * 2 + 1] = c.uv[o * 2 + 1]; }
}
// cloud_fill_kernel with the pose of `local` from the record of the pixel's slice: a sibling, so that the kernel above stays what it was
__global__ __launch_bounds__(kCloudBlock) void cloud_fill_rolling_kernel(const CloudFillParams c, const CloudRollParams r)
{
    const int lane = (int)threadIdx.x & 63;
    const int64_t chunk = (int64_t)blockIdx.x * (kCloudBlock / kCloudChunk) + ((int)threadIdx.x >> 6);
    if (chunk >= (int64_t)c.nchunks) return;                    // (wave-uniform)
    const int32_t frame = (int32_t)chunk / c.chunks_per_frame;
    const int64_t at = (int64_t)((int32_t)chunk - frame * c.chunks_per_frame) * kCloudChunk + lane;
    const unsigned long long b = c.keep[chunk];                 // the count kernel's ballot
    if (at >= c.px || !((b >> lane) & 1ull)) return;
    // kept lanes below this one: v_mbcnt_lo / v_mbcnt_hi of the ballot
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    const unsigned long long slot = (unsigned long long)c.chunk_offsets[chunk] + below;
    if (slot >= (unsigned long long)c.capacity) return;
    const size_t o = (size_t)frame * (size_t)c.px + (size_t)at, j = (size_t)slot;
    if (c.range) c.range[j] = c.t[o];
    if (c.pixel) c.pixel[j] = (int32_t)at;
    if (c.frame) c.frame[j] = frame;
    if (c.out_instance) c.out_instance[j] = c.instance[o];
    if (c.out_triangle) c.out_triangle[j] = c.triangle[o];
    if (c.position || c.local) {
        const V3 loc = v3(c.location[o * 3], c.location[o * 3 + 1], c.location[o * 3 + 2]);
        if (c.position) { c.position[j * 3] = loc.x; c.position[j * 3 + 1] = loc.y; c.position[j * 3 + 2] = loc.z; }
        if (c.local) {
            // rule 5 with the pose of the pixel's slice
            const int32_t px_y = (int32_t)(at / (int64_t)r.width), px_x = (int32_t)(at - (int64_t)px_y * (int64_t)r.width);
            int32_t slice = (r.axis ? px_y : px_x) / r.slice_pixels;
            slice = slice < r.slices ? slice : r.slices - 1;
            const RollRecord& rec = r.records[(size_t)frame * (size_t)r.slices + (size_t)slice];
            const V3 l = apply_quat(rec.q_pose, v3(loc.x - rec.origin[0], loc.y - rec.origin[1], loc.z - rec.origin[2]));
            c.local[j * 3] = l.x; c.local[j * 3 + 1] = l.y; c.local[j * 3 + 2] = l.z;
        }
    }
    if (c.out_normal) { c.out_normal[j * 3] = c.normal[o * 3]; c.out_normal[j * 3 + 1] = c.normal[o * 3 + 1]; c.out_normal[j * 3 + 2] = c.normal[o * 3 + 2]; }
    if (c.out_uv) { c.out_uv[j * 2] = c.uv[o * 2]; c.out_uv[j * 2 + 1] = c.uv[o * 2 + 1]; }
}

// ---------------------------------------------------------------------------------------------------------
// Extension kernel (rt_render_ex): samples per pixel, specular bounces, and the sun + shadow pass that the reference
// carries as commented-out code (raycast.cu:249-290).  The reference has no implementation of these, so the
// semantics are defined in DESIGN.md section 7 (and restated by the test oracle); with spp = 1, bounces = 0, lighting = 0 the
// result equals render_kernel's bit for bit.
// ---------------------------------------------------------------------------------------------------------
// LOC: keep the accepted hit's world location (secondary rays start there).  ANYHIT: a shadow ray, cast_ray(..., true, FLT_MAX)
// of raycast.cu:272 -- it returns at its first accepted hit (:129-133), i.e. a lane that has one (then, and only then, its
// hit.min is below FLT_MAX) takes no part in the remaining instances.
// OPTIMISTIC: only the samples-only kernel asks for it -- in the bounce kernel, which carries its path state across the casts in
// registers it does not have, the second loop costs more in spills than the branches it saves: c3 +8 %
// (profiles/r05_experiments/ex_one_wave_workgroups.log).
// VIEW (the samples-only kernel's primary rays: they share the frame's origin): the cast reads view records, see trace_loop.
// PRIMARY: the ray starts at the camera in every lane (trace_instance's UNIFORM_ORG).
// SEC: a ray with an origin of its own per lane through the hand-written loop (trace_instance: the ray queries); with OCTANTS and OPTIMISTIC.
// tmax (ANYHIT): the light distance of raycast.cu:129-133 -- a lane is done at its first accepted hit below it, and the instance loops
// skip the instances after that hit (FLT_MAX for the extension's shadow rays, per ray for rt_occluded).
// Whether the cast has returned: a hit was accepted below tmax.  (hit.min starts at FLT_MAX, which is below a tmax of +inf without any
// hit; for tmax <= FLT_MAX -- the shadow rays' constant among them -- `hit.min < tmax` alone says it.)
__device__ __forceinline__ bool any_hit_done(const Hit& hit, float tmax)
{
    return hit.min < tmax && (tmax <= FLT_MAX || hit.instance >= 0);
}
template <bool LOC = true, bool OCTANTS = false, bool ANYHIT = false, class STK = Stack, bool OPTIMISTIC = false, bool VIEW = false, bool PRIMARY = false, bool SEC = false>
__device__ __forceinline__ Hit cast_ray_ex(const RenderParams& p, V3 org, V3 dir, STK& stack, int& pops, float tmax = FLT_MAX)
{
    static_assert(!VIEW || OPTIMISTIC, "view records are read by the LDS-only loops");
    static_assert(!SEC || (OCTANTS && OPTIMISTIC && !VIEW && !PRIMARY), "SEC");
    Hit hit;
    hit.min = FLT_MAX; hit.slot = -1; hit.instance = -1; hit.u = 0.0f; hit.v = 0.0f;
    hit.loc = v3(0.0f, 0.0f, 0.0f);
    Counters<false> none;
    if constexpr (OPTIMISTIC && STK::kSpill) {
        // the optimistic stack (StackT, render_pixel): the cast on the LDS part alone, and again from its start on the general stack
        // for the lanes whose stack outgrew it (their pop count starts again too)
        StackT<STK::kStride, false, true> fast;
        fast.lds = stack.lds; fast.spill = nullptr; fast.lds_depth = stack.lds_depth; fast.sp = 0;
        const int pops_before = pops;
        int outgrown = 0;
        for (int i = 0; i < p.num_instances; i++) {
            if constexpr (ANYHIT) { if (any_hit_done(hit, tmax)) continue; }
            trace_instance<false, false, LOC, false, StackT<STK::kStride, false, true>, true, OCTANTS, ANYHIT, VIEW, PRIMARY, false, SEC>(p, p.instances[i], i, org, dir, fast, hit, none,
                                                                                                                                        nullptr, &pops, p.view_base, tmax);
            // (a shadow ray that found its hit left the loop with entries on its stack: it is done, not outgrown)
            outgrown |= (ANYHIT && SEC && any_hit_done(hit, tmax)) ? 0 : fast.sp;
        }
        if (outgrown == 0) return hit;
        pops = pops_before;
        hit.min = FLT_MAX; hit.slot = -1; hit.instance = -1; hit.u = 0.0f; hit.v = 0.0f;
        hit.loc = v3(0.0f, 0.0f, 0.0f);
    }
    for (int i = 0; i < p.num_instances; i++) {
        if constexpr (ANYHIT) { if (any_hit_done(hit, tmax)) continue; }
        trace_instance<false, false, LOC, false, STK, true, OCTANTS, ANYHIT>(p, p.instances[i], i, org, dir, stack, hit, none, nullptr, &pops, 0u, tmax);
    }
    return hit;
}

// world normal of the accepted hit, raycast.cu:115-122
__device__ __forceinline__ V3 hit_normal(const RenderParams& p, const Hit& hit)
{
    const DevInstance& in = p.instances[hit.instance];
    const float4* t = p.records + (size_t)hit.slot * 4;
    float4 t0 = t[0], t1 = t[1];
    V3 n = apply_quat(in.q_inv_rot, v3(t0.w, t1.x, t1.y));
    n.x *= in.scale[0]; n.y *= in.scale[1]; n.z *= in.scale[2];
    return normalize(n);
}

// One workgroup = one 16x16 tile of ONE sample index (blockIdx.y): every (pixel, sample) pair has its own random
// stream, so the samples of a pixel are independent work items and a frame of spp samples is dispatched like a batch
// of spp frames.  (A pixel's samples used to run as a loop inside its lane: the waves on the silhouette then lived
// 64 x as long as their neighbours and the kernel spent most of its time waiting for a handful of them.)
// The sample's radiance and node pops go to ex_samples[sample][local pixel]; resolve_ex_kernel sums them in order.
// (8 waves per SIMD at 32 spilled registers beats 7 / 6 / 5 waves with 18 / 4 / 0 spills: +2 % / +8 % / +21 % time.)
// SIMPLE = no bounces and no lighting (samples per pixel only, BASELINE configs[3]): the path is one primary ray, so
// nothing but the hit has to survive the cast -- no path state spilled around the traversal loop, no hit location.
// PX = the samples of a pixel share a wave (the default for 4 and more samples per pixel): a wave is px_pw x px_ph pixels
// times px_n sample slots -- 2 x 2 pixels x 16 samples, or 1 pixel x 64 samples -- instead of 8 x 8 pixels of one sample
// index.  The jittered rays of one pixel visit almost the same nodes in almost the same order, so the lanes of a wave stay
// together through the loop (most iterations find every lane holding the same entry and take the scalar fetch) and finish
// together; and because a pixel's samples now sit in one wave, they are added up -- in sample order, by one lane per channel,
// through the wave's own LDS columns -- right here: no sample planes in HBM, no resolve pass.  Frames of more than 64 samples
// take several launches, the running sums wait in ex_acc in between.  What a (pixel, sample) pair computes does not depend on
// the lane it runs in, so the frame is the same bit for bit (tests/test_gpu_parity.py compares the two mappings).
// (8 waves per SIMD stays the best residency with this mapping too: 7 / 6 / 5 waves +1.6 % / +6 % / +17 % on c3, +4 % on c4)
// Which (pixel, sample) pair thread `tid` of workgroup (tile, row) works on.  A function of its own so that the kernel can call
// it again after the casts instead of keeping the results (see render_pixel: registers the traversal loop has no room for).
template <bool PX>
__device__ __forceinline__ void ex_work_item(const RenderParams& p, int tile, int row, int tid, int& x, int& ly, int& y, int& s, bool& valid)
{
    const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    const int wave = tid >> 6, lane = tid & 63;
    if constexpr (PX) {
        const int pix = lane / p.px_n, sl = lane % p.px_n;
        x = tx * 2 * p.px_pw + (wave & 1) * p.px_pw + pix % p.px_pw;
        ly = ty * 2 * p.px_ph + (wave >> 1) * p.px_ph + pix / p.px_pw;
        s = p.sample_base + sl;
        valid = x < p.width && ly < p.local_rows && sl < p.px_count;
    } else {
        x = tx * kTile + (wave & 1) * 8 + (lane & 7);
        ly = ty * kTile + (wave >> 1) * 8 + (lane >> 3);
        s = p.sample_base + row;
        valid = x < p.width && ly < p.local_rows;
    }
    y = ly;                                                     // stripes: local -> frame row (the identity for one rank)
    if (p.num_ranks != 1) y = ((ly / p.stripe_rows) * p.num_ranks + p.rank) * p.stripe_rows + ly % p.stripe_rows;
}

// The random stream of (pixel, sample) after `drawn` values: the reference's per-pixel seed (raycast.cu:190: int idx * 1000)
// plus the sample index.  A path does not carry the six words of its stream across its casts; it carries how many values
// it has drawn and steps a fresh copy forward when it next needs one (a few dozen integer operations against the hundreds
// of a cast; the sequence of values is the same).
__device__ __forceinline__ Xorwow ex_stream(const RenderParams& p, int x, int y, int s, int drawn)
{
    Xorwow rng;
    xorwow_init(rng, (unsigned long long)((long long)(int32_t)((uint32_t)(y * p.width + x) * 1000u) + (long long)s));
    for (int k = 0; k < drawn; k++) (void)xorwow_next(rng);
    return rng;
}

// One wave per workgroup (round 5, like the primary kernels: a wave's slot is refilled when the wave ends, not when the last of
// four does): workgroups 4t .. 4t + 3 are the four waves of tile t, and `quarter` below is what the wave index within a 256-thread
// workgroup used to be.
constexpr int kExBlock = 64;
typedef StackT<kExBlock> ExStack;
// The bounce kernel is compiled for eight waves per SIMD (64 registers) and its shadow and bounce rays take the compiler's loop.  Through
// the hand-written loop (trace_instance's SEC, which the ray queries ship) they need 53 registers at the cast site: at eight waves that
// pushes the path state into scratch (c3 +5 %), and every wave given up for registers costs more than the loop returns
// (profiles/r06_experiments/ex_secondary_asm.md).
constexpr int kExBounceWaves = 8;
template <bool SIMPLE, bool PX = false, bool VIEW = false>
__global__ __launch_bounds__(kExBlock, (SIMPLE ? 8 : kExBounceWaves)) void render_ex_kernel(const RenderParams p)
{
    extern __shared__ int lds_stack[];
    const FrameParams& f = p.frames[0];
    const unsigned bx = blockIdx.x;
    const int tile = (int)(bx >> 2), quarter = (int)(bx & 3);
    int x, ly, y, s;
    bool valid;
    ex_work_item<PX>(p, tile, (int)blockIdx.y, quarter * 64 + (int)threadIdx.x, x, ly, y, s, valid);
    if constexpr (!PX) { if (!valid) return; }
    unsigned long long t_start = 0;
    if (p.trace) t_start = wall_clock64();

    int spill[kMaxStack - kLdsStack];
    ExStack stack;
    // (the thread's index lives on as the address of its LDS stack column only)
    stack.lds = (lds_int*)lds_stack + threadIdx.x; stack.spill = spill; stack.lds_depth = lds_rows(p.stack_depth); stack.sp = 0;
    auto where = [&](int& x_, int& ly_, int& y_, int& s_, bool& valid_) {
        asm volatile("" : "+v"(stack.lds));                     // (hides the address's origin: the optimiser would keep the first results alive)
        ex_work_item<PX>(p, tile, (int)blockIdx.y, quarter * 64 + (int)(stack.lds - (lds_int*)lds_stack), x_, ly_, y_, s_, valid_);
    };
    int pops = 0;
    V3 sample = v3(0.0f, 0.0f, 0.0f);
    if (valid) {

    const V3 sun = normalize(v3(-0.2f, 0.0f, 1.0f));                                                    // raycast.cu:249-250
    float px = (float)x, py = (float)y;
    int drawn = 0;                                              // values taken from the (pixel, sample) stream so far
    if (s > 0) {
        Xorwow rng = ex_stream(p, x, y, s, 0);
        px = px + (xorwow_uniform(rng) - 0.5f); py = py + (xorwow_uniform(rng) - 0.5f);
        drawn = 2;
    }
    V3 org = v3(f.origin[0], f.origin[1], f.origin[2]);
    V3 dir = world_direction(f, camera_space_direction(f, px, py));
    V3 weight = v3(1.0f, 1.0f, 1.0f);
    if constexpr (SIMPLE) {                                     // the loop below for bounces = 0, lighting = 0, written out
        const Hit hit = cast_ray_ex<false, true, false, ExStack, true, VIEW, true>(p, org, dir, stack, pops);
        if (hit.min == FLT_MAX) sample = sample + weight * v3(1.0f, 0.8f, 0.6f);
        else {
            const V3 base = base_colour(p, hit);
            float illum = 1.0f;
            illum = fminf(1.0f, illum);
            illum = fmaxf(0.4f, illum);
            const V3 local = v3(illum * base.x, illum * base.y, illum * base.z);
            sample = sample + weight * (local * (1.0f - 0.0f));
        }
    } else
    {
    // one depth of the path: cast, shade, reflect; false = the path has ended
    // (`primary` = std::true_type for the camera ray.  In the VIEW form of this kernel -- launched when the frame qualifies for view
    // records, i.e. when the tree is small beside the frame -- it takes the hand-written loop and the frame's view: c3 / c5 -4.5 %.
    // The other form keeps the compiler's loop for it: without a view the camera ray's gain is smaller than what 18 more spilled
    // registers cost the bounce casts -- c6 with mirror walls, whose 4 M-node tree gets no view, lost 9 % with it.)
    // (after_cast: everything a depth does with the hit of its cast)
    auto after_cast = [&](Hit hit, const int depth) __attribute__((always_inline)) -> bool {
        if (hit.min == FLT_MAX) { sample = sample + weight * v3(1.0f, 0.8f, 0.6f); return false; }
        float illum = 1.0f;
        // (base colour, normal and cosine are kept across the shadow cast: deriving them again after it from (slot, instance, u, v) gives
        // the same bits with fewer spilled registers and is 1.1 % slower on c3, profiles/r05_experiments/ex_spill_variants.md)
        const V3 base = base_colour(p, hit);
        const V3 n = hit_normal(p, hit);
        if (p.lighting) {                                   // raycast.cu:249-287 with the commented lines active
            const float cos_illum = dot(n, sun);
            illum = (float)(0.4 * (double)cos_illum);
            if (dot(n, sun) > 0) {
                // (only hit-or-miss survives a shadow cast: no hit location to keep.  Octant loops at either cast of this
                // kernel: within +-0.6 %, profiles/r04_experiments/octants_in_extension_kernels.log)
                const Hit sh = cast_ray_ex<false, false, true, ExStack>(p, hit.loc + sun * (float)1e-4, sun, stack, pops);
                if (sh.min == FLT_MAX) illum = (float)(1.0 * (double)cos_illum);
            }
        }
        illum = fminf(1.0f, illum);                         // raycast.cu:289-290
        illum = fmaxf(0.4f, illum);
        const V3 local = v3(illum * base.x, illum * base.y, illum * base.z);
        const DevMaterial& mat = p.materials[p.instances[hit.instance].material_index];
        const float m = depth < p.bounces ? mat.metallic : 0.0f;
        sample = sample + weight * (local * (1.0f - m));
        if (!(m > 0.0f)) return false;
        weight = weight * (base * m);
        const float k = 2.0f * dot(dir, n);
        V3 r = dir - n * k;
        if (mat.roughness > 0.0f) {
            int x_, ly_, y_, s_; bool v_;
            where(x_, ly_, y_, s_, v_);
            Xorwow rng = ex_stream(p, x_, y_, s_, drawn);
            drawn += 3;
            float rx = 2.0f * xorwow_uniform(rng) - 1.0f, ry = 2.0f * xorwow_uniform(rng) - 1.0f, rz = 2.0f * xorwow_uniform(rng) - 1.0f;
            r = r + v3(rx, ry, rz) * mat.roughness;
        }
        r = normalize(r);
        org = hit.loc + r * (float)1e-4;
        dir = r;
        return true;
    };
    auto step = [&](auto primary, const int depth) __attribute__((always_inline)) -> bool {
        constexpr bool kPrimary = VIEW && decltype(primary)::value;
        Hit hit = cast_ray_ex<true, kPrimary, false, ExStack, kPrimary, kPrimary, kPrimary>(p, org, dir, stack, pops);
        return after_cast(hit, depth);
    };
    // the primary ray's depth written out: weight = 1 and sample = 0 are constants across its cast, not registers to keep
    // (-0.7 % on c3, profiles/r05_experiments/ex_spill_variants.md)
    if (step(std::true_type{}, 0))
        for (int depth = 1; depth <= p.bounces; depth++) if (!step(std::false_type{}, depth)) break;
    }
    }
    where(x, ly, y, s, valid);
    const int lane = (int)(stack.lds - (lds_int*)lds_stack);
    if constexpr (PX) {
        // the wave's samples -> its LDS columns (the traversal stacks are idle now), four rows of 64 words: r g b pops
        lds_int* mine = (lds_int*)lds_stack;
        mine[0 * kExBlock + lane] = __float_as_int(sample.x);
        mine[1 * kExBlock + lane] = __float_as_int(sample.y);
        mine[2 * kExBlock + lane] = __float_as_int(sample.z);
        mine[3 * kExBlock + lane] = pops;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the first four lanes of a pixel add up one channel each, in sample order (what resolve_ex_kernel does per pixel)
        const int c = lane % p.px_n;
        if (c < 4 && x < p.width && ly < p.local_rows) {
            const lds_int* col = mine + c * kExBlock + (lane - c);
            const size_t pixel = (size_t)ly * p.width + x;
            if (c < 3) {
                float acc = 0.0f;
                if (!p.px_first) acc = ((const float*)&p.ex_acc[pixel])[c];
                for (int k = 0; k < p.px_count; k++) acc = acc + __int_as_float(col[k]);
                if (!p.px_last) ((float*)&p.ex_acc[pixel])[c] = acc;
                else (f.img + (size_t)ly * p.pitch + 3 * (size_t)x)[c] = to_u8(acc / (float)p.spp * 255.0f);
            } else {
                int acc = 0;
                if (!p.px_first) acc = __float_as_int(p.ex_acc[pixel].w);
                for (int k = 0; k < p.px_count; k++) acc += col[k];
                if (!p.px_last) ((int*)&p.ex_acc[pixel])[3] = acc;
                else if (p.total_pops) p.total_pops[(size_t)y * p.width + x] = acc;
            }
        }
    } else
    p.ex_samples[(size_t)blockIdx.y * ((size_t)p.local_rows * p.width) + (size_t)ly * p.width + x] =
        make_float4(sample.x, sample.y, sample.z, __int_as_float(pops));
    if (p.trace) {                                              // diagnostic: per-wave lifetime (RT_TRACE_FILE)
        const unsigned long long active = __ballot(true);
        if (lane == __ffsll((long long)active) - 1) {
            unsigned long long* t = p.trace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16;
            t[0] = t_start; t[1] = wall_clock64(); t[3] = (unsigned long long)tile;
        }
    }
}

// pixel = u8(sum of its samples in index order / spp * 255); a frame with many samples arrives in several chunks of
// `count` samples, the running sum (and node-pop total) waits in ex_acc in between.
__global__ void resolve_ex_kernel(const RenderParams p, int count, int first, int last)
{
    const size_t npix = (size_t)p.local_rows * p.width;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    V3 acc = v3(0.0f, 0.0f, 0.0f);
    int pops = 0;
    if (!first) { const float4 a = p.ex_acc[i]; acc = v3(a.x, a.y, a.z); pops = __float_as_int(a.w); }
    for (int k = 0; k < count; k++) {
        const float4 q = p.ex_samples[(size_t)k * npix + i];
        acc = acc + v3(q.x, q.y, q.z);
        pops += __float_as_int(q.w);
    }
    if (!last) { p.ex_acc[i] = make_float4(acc.x, acc.y, acc.z, __int_as_float(pops)); return; }
    const int ly = (int)(i / p.width), x = (int)(i % p.width);
    const int y = ((ly / p.stripe_rows) * p.num_ranks + p.rank) * p.stripe_rows + ly % p.stripe_rows;
    const float nspp = (float)p.spp;
    uint8_t* out = p.frames[0].img + (size_t)ly * p.pitch + 3 * (size_t)x;
    out[0] = to_u8(acc.x / nspp * 255.0f);
    out[1] = to_u8(acc.y / nspp * 255.0f);
    out[2] = to_u8(acc.z / nspp * 255.0f);
    if (p.total_pops) p.total_pops[(size_t)y * p.width + x] = pops;
}

// rows of a rank-major gathered buffer back into frame order (rt_unstripe): a plain row copy, T = uint4 when every
// address involved is 16-byte aligned (the usual case: tight or hipMallocPitch pitches), bytes otherwise.
template <class T>
__global__ void unstripe_kernel(const uint8_t* __restrict__ src, size_t local_pitch, size_t rank_stride, size_t src_frame_stride,
                                uint8_t* __restrict__ dst, size_t pitch, size_t dst_frame_stride, int row_units, int height,
                                int stripe_rows, int num_ranks, int rotate_first)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;     // unit i of the frame: row i / row_units
    const int y = (int)(i / (size_t)row_units), u = (int)(i % (size_t)row_units);
    if (y >= height) return;
    src += (size_t)blockIdx.z * src_frame_stride;               // blockIdx.z = frame of the batch
    dst += (size_t)blockIdx.z * dst_frame_stride;
    const int stripe = y / stripe_rows;
    int rank = stripe % num_ranks;                              // the stripe's owner ...
    // ... which, when ownership rotates with the frame index (rt_render_stripes_batch_rotating), rank r plays for frame index fi
    // iff (r + fi) % num_ranks == owner
    if (rotate_first >= 0) rank = (rank + num_ranks - (rotate_first + (int)blockIdx.z) % num_ranks) % num_ranks;
    const int ly = (stripe / num_ranks) * stripe_rows + y % stripe_rows;
    const T* s = (const T*)(src + (size_t)rank * rank_stride + (size_t)ly * local_pitch);
    T* d = (T*)(dst + (size_t)y * pitch);
    d[u] = s[u];
}

// Heavy-first dispatch order of the next single-frame (or thin striped) launch: a counting sort of the tiles by cost -- the loop
// iterations of the longest lane among the tile and its neighbours in the launches since the last sort, longest first.  A tile's key is
// computed once and kept (a render on another stream may be rewriting the costs): whatever the values, the result is a permutation
// of the tiles.  The sort runs on the scene's side stream, but a hipDeviceSynchronize waits for it like for everything else -- the
// reference's loop synchronises the device every two frames (kernel.cu:279) -- so it has to be short AND has to get going: every
// thread loads eight costs before it touches any of them (one memory latency per 2048 tiles).
constexpr int kSortKeys = 1024, kSortThreads = 256, kSortBatch = 8;
// Round 6: ONE workgroup of 256 threads (was 1 024).  Primary launches are one-wave workgroups that refill a wave slot the moment it
// falls free; a 1 024-thread workgroup needs sixteen free slots on ONE compute unit at the same moment, which a saturated chip offers
// when the frames END -- the sort then ran after them, and a device synchronise (the reference's loop: one every two frames) waited
// for it.  Four waves find room within microseconds.  The costs arrive as neighbourhood maxima (render_kernel<.., ORDERED>), so the
// sort reads one value per tile; it clears what it has read (the launches accumulate maxima).
__global__ __launch_bounds__(kSortThreads) void tile_sort_kernel(int32_t* cost, int ntiles, int32_t* __restrict__ keys, int32_t* __restrict__ order)
{
    constexpr int kPer = kSortKeys / kSortThreads;              // classes per thread in the scan
    static_assert(kSortKeys % kSortThreads == 0, "whole classes per thread");
    __shared__ int count[kSortKeys], scan[kSortThreads];
    const int t = threadIdx.x;
    for (int c = t; c < kSortKeys; c += kSortThreads) count[c] = 0;
    __syncthreads();
    for (int base = 0; base < ntiles; base += kSortThreads * kSortBatch) {
        int k[kSortBatch];
#pragma unroll
        for (int j = 0; j < kSortBatch; j++) {
            const int i = base + j * kSortThreads + t;
            k[j] = i < ntiles ? cost[i] : -1;                   // iterations of the longest lane (a few hundred at most) of the 3 x 3 tiles around i
            if (i < ntiles) cost[i] = 0;                        // (a launch running beside this sort may lose a cost it had just written: that
                                                                // tile is ordered by its neighbours' and earlier frames' costs, or late, once)
        }
#pragma unroll
        for (int j = 0; j < kSortBatch; j++) {
            const int i = base + j * kSortThreads + t;
            if (i < ntiles) {
                int c = k[j] < 0 ? 0 : (k[j] > kSortKeys - 1 ? kSortKeys - 1 : k[j]);
                c = kSortKeys - 1 - c;                          // longest first
                keys[i] = c;
                atomicAdd(&count[c], 1);
            }
        }
    }
    __syncthreads();
    // exclusive prefix over the classes (each thread its kPer consecutive classes, Hillis-Steele over the threads' sums): count[]
    // becomes the running cursor of each class
    int own[kPer], mine = 0;
#pragma unroll
    for (int c = 0; c < kPer; c++) { own[c] = count[t * kPer + c]; mine += own[c]; }
    scan[t] = mine;
    __syncthreads();
    for (int o = 1; o < kSortThreads; o <<= 1) {
        const int v = t >= o ? scan[t - o] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    int at = scan[t] - mine;
#pragma unroll
    for (int c = 0; c < kPer; c++) { count[t * kPer + c] = at; at += own[c]; }
    __syncthreads();
    for (int base = 0; base < ntiles; base += kSortThreads * kSortBatch) {
        int k[kSortBatch];
#pragma unroll
        for (int j = 0; j < kSortBatch; j++) {
            const int i = base + j * kSortThreads + t;
            k[j] = i < ntiles ? keys[i] : 0;                    // (this thread's own stores of the first pass)
        }
#pragma unroll
        for (int j = 0; j < kSortBatch; j++) {
            const int i = base + j * kSortThreads + t;
            if (i < ntiles) order[atomicAdd(&count[k[j]], 1)] = i;
        }
    }
}

// ---- refit of a deforming mesh (rt_scene_refit_mesh): same topology, new vertex positions ----------------------------
// The reference has no refit (it can only re-pose instances, Scene.cpp:67-74); SURVEY.md 8(f) item 2 lists it next to the
// build.  Result = the tree BVHTree::fill's bounds pass (BVHTree.hpp:206-209) would give every node of the SAME tree over
// the moved triangles: a node's box is the exact min / max over its triangles' vertices, so folding children's boxes
// bottom-up gives the same values as folding the triangles.
__global__ void refit_triangles_kernel(float4* __restrict__ records, const int32_t* __restrict__ tri_id, int slot_base, int num_slots,
                                       const float* __restrict__ vertices, const float* __restrict__ normals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_slots) return;
    const int slot = slot_base + i;
    const int t = tri_id[slot];
    const float* v = vertices + 9 * (size_t)t;
    const float* nn = normals + 3 * (size_t)t;
    const V3 v0 = v3(v[0], v[1], v[2]), v1 = v3(v[3], v[4], v[5]), v2 = v3(v[6], v[7], v[8]);
    const V3 e0 = v2 - v0, e1 = v1 - v0;                        // TrianglePrimitive.hpp:154-155 (as rt_scene_upload)
    const float d00 = dot(e0, e0), d01 = dot(e0, e1), d11 = dot(e1, e1);
    const float inv = 1.0f / (d00 * d11 - d01 * d01);          // TrianglePrimitive.hpp:164
    float4* q = records + (size_t)slot * 4;
    q[0] = make_float4(v0.x, v0.y, v0.z, nn[0]);
    q[1] = make_float4(nn[1], nn[2], e0.x, e0.y);
    q[2] = make_float4(e0.z, e1.x, e1.y, e1.z);
    q[3] = make_float4(d00, d01, d11, inv);
}

// box of the subtree behind `ref`: a leaf's triangles' vertices, or the union of the two boxes an interior record holds
__device__ __forceinline__ void refit_child_box(const float4* records, const int32_t* tri_id, const int32_t* leaf_count, const float* vertices,
                                                int32_t ref, float* mn, float* mx)
{
    for (int c = 0; c < 3; c++) { mn[c] = FLT_MAX; mx[c] = -FLT_MAX; }
    if (ref >= 0) {
        const float4* q = records + (size_t)ref * 4;
        const float4 q0 = q[0], q1 = q[1], q2 = q[2];
        const float a[6] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y}, b[6] = {q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        for (int c = 0; c < 3; c++) { mn[c] = fminf(fminf(mn[c], a[c]), b[c]); mx[c] = fmaxf(fmaxf(mx[c], a[3 + c]), b[3 + c]); }
    } else {
        const int slot = ref & kSlotMask;
        int count = (ref >> kSlotBits) & 31;
        if (count == 31) count = leaf_count[slot];
        for (int k = 0; k < count; k++) {
            const float* v = vertices + 9 * (size_t)tri_id[slot + k];
            for (int j = 0; j < 3; j++)
                for (int c = 0; c < 3; c++) { mn[c] = fminf(mn[c], v[3 * j + c]); mx[c] = fmaxf(mx[c], v[3 * j + c]); }
        }
    }
}

// one level of interior nodes, deepest level first: sched[begin .. end) are the record indices of the level
__global__ void refit_level_kernel(float4* records, const int32_t* __restrict__ tri_id, const int32_t* __restrict__ leaf_count,
                                   const float* __restrict__ vertices, const int32_t* __restrict__ sched, int begin, int end, int32_t* mesh_flag)
{
    const int i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end) return;
    float4* q = records + (size_t)sched[i] * 4;
    const float4 q3 = q[3];
    float amn[3], amx[3], bmn[3], bmx[3];
    refit_child_box(records, tri_id, leaf_count, vertices, __float_as_int(q3.x), amn, amx);
    refit_child_box(records, tri_id, leaf_count, vertices, __float_as_int(q3.y), bmn, bmx);
    q[0] = make_float4(amn[0], amn[1], amn[2], amx[0]);
    q[1] = make_float4(amx[1], amx[2], bmn[0], bmn[1]);
    q[2] = make_float4(bmn[2], bmx[0], bmx[1], bmx[2]);
    const float w[12] = {amn[0], amn[1], amn[2], amx[0], amx[1], amx[2], bmn[0], bmn[1], bmn[2], bmx[0], bmx[1], bmx[2]};
    if (!boxes_ordered(w)) *mesh_flag = kBoxUnordered;          // (cleared by refit_mesh before the first level: a refit rewrites every interior record)
}

// A run of consecutive NARROW levels (the top of every tree, and the thin bottom of a deep one: each a launch of a few dozen
// threads otherwise) in one launch of one workgroup: level after level with a barrier in between.  Children written by
// this workgroup are read by this workgroup only, so the barrier orders them.
constexpr int kRefitRunLevels = 32, kRefitRunThreads = 256;
struct RefitRun { int32_t levels; int32_t bound[kRefitRunLevels + 1]; };       // level k of the run = sched[bound[k] .. bound[k + 1])
__global__ __launch_bounds__(kRefitRunThreads) void refit_run_kernel(float4* records, const int32_t* __restrict__ tri_id,
                                                                   const int32_t* __restrict__ leaf_count, const float* __restrict__ vertices,
                                                                   const int32_t* __restrict__ sched, const RefitRun run, int32_t* mesh_flag)
{
    for (int l = 0; l < run.levels; l++) {
        for (int i = run.bound[l] + (int)threadIdx.x; i < run.bound[l + 1]; i += kRefitRunThreads) {
            float4* q = records + (size_t)sched[i] * 4;
            const float4 q3 = q[3];
            float amn[3], amx[3], bmn[3], bmx[3];
            refit_child_box(records, tri_id, leaf_count, vertices, __float_as_int(q3.x), amn, amx);
            refit_child_box(records, tri_id, leaf_count, vertices, __float_as_int(q3.y), bmn, bmx);
            q[0] = make_float4(amn[0], amn[1], amn[2], amx[0]);
            q[1] = make_float4(amx[1], amx[2], bmn[0], bmn[1]);
            q[2] = make_float4(bmn[2], bmx[0], bmx[1], bmx[2]);
            const float w[12] = {amn[0], amn[1], amn[2], amx[0], amx[1], amx[2], bmn[0], bmn[1], bmn[2], bmx[0], bmx[1], bmx[2]};
            if (!boxes_ordered(w)) *mesh_flag = kBoxUnordered;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// rt_scene_update_instance_async: the new record travels as a kernel argument, so the update is ordered on the stream
// like any launch and needs no host buffer that outlives the call
__global__ void set_instance_kernel(DevInstance* dst, const DevInstance value) { *dst = value; }

// View records of the frames of one launch (RtScene::ViewPool, trace_loop<.., VIEW>): for every frame and every
// instance, the instance's interior records with `box - origin` in place of the twelve box words -- origin = the frame's camera
// position in the instance's mesh space, computed by the function the traversal uses (to_mesh_space), the subtraction being
// the one box_differences does per visit: the same fp32 operation on the same operands, done once.  One thread per 16 bytes of a
// record, for kViewFrameChunk frames of the launch in turn (blockIdx.y = the chunk): what does not depend on the frame -- the record's
// words, the triangles the cull below looks at -- is read once per chunk, a wave's stores of one frame are one run of 1 KiB, and the
// origins of the chunk's frames, one per instance, are computed once per workgroup (LDS) instead of once per thread.
// In front of a frame's view records stand its ray headers (RayHeader, rt_device_types.h), one 64-byte block per instance, written
// by one thread each: that same origin and the instance fields a wave of render_kernel<.., VIEW> needs before its loop.
struct ViewJob {
    int32_t n;                                  // instances
    int32_t first[kMaxViewInstances];           // first record of the instance's part of a frame's view
    int32_t node_base[kMaxViewInstances];       // first interior record of the instance's mesh
    int32_t count[kMaxViewInstances];           // interior-record capacity of that mesh
    int32_t total;                              // records to write per frame (sum of count)
    // the launch's direction table (RenderParams::dir_table; 0 blocks = none): workgroups record_blocks .. of every row of the grid
    // write it, `dir_blocks` per row, four 8x8 tiles each -- every row takes a share, so no row brings workgroups with nothing to do
    uint32_t record_blocks, dir_blocks;
    // back-facing leaves: 1 = the views of this launch are read by kernels that report no visit counts -- a leaf child
    // none of whose triangles can be accepted from the frame's origin gets a box that no ray passes.  0 = boxes as they are.
    int32_t cull;
    uint32_t records_end;                       // records of the scene: a leaf reference is followed only below it
};

// Back-facing leaves.  A candidate is accepted only with denom < 0 and !(tt < 0), tt = N / denom, N = (v0 - ro) . n: N depends on the
// frame's origin and the triangle alone.  With N >= kCullMin and denom < 0, tt < 0 strictly -- 2^-20 / |denom| is above 2^-149 for every
// finite denom, and the IEEE division does not round it to -0; an infinite denom gives -0 and a NaN point.
constexpr float kCullMin = 9.5367431640625e-07f;        // 2^-20
static_assert(kCullMin * 1048576.0f == 1.0f, "2^-20");
// the six box words of a culled child: a quiet NaN with a payload that no subtraction produces (rt_scene_view_cull_stats looks for it)
constexpr int kCullWord = 0x7fc0c011;

// What triangle k of the leaf child `ref` says about culling that child, whatever the frame: kCullKeeps for anything that is not a leaf
// of one to four coded triangles (interior nodes, empty leaves, leaves whose count is looked up or above four are left alone),
// kCullSilent for k beyond the leaf's count, kCullAsk for a triangle to evaluate per frame -- v0 and the normal are then in t0, t1.
constexpr int kCullKeeps = 0, kCullSilent = 1, kCullAsk = 2;
__device__ __forceinline__ int cull_triangle(const RenderParams& p, const ViewJob& job, int32_t ref, int k, float4& t0, float4& t1)
{
    const int coded = (ref >> kSlotBits) & 31;
    const uint32_t slot = (uint32_t)(ref & kSlotMask);
    if (ref >= 0 || coded < 1 || coded > 4 || slot + (uint32_t)coded > job.records_end) return kCullKeeps;
    if (k >= coded) return kCullSilent;
    const float4* t = p.records + (size_t)(slot + (uint32_t)k) * 4;
    t0 = t[0]; t1 = t[1];
    return kCullAsk;
}
// "This triangle keeps its leaf alive for the frame whose origin is o": !(N >= kCullMin), N from the hand-written loop's own operations
// in their order (RT_ASM_LOOP_TEXT "numerator"; dot(v0 - r.ro, nrm) in triangle_test)
__device__ __forceinline__ bool cull_keeps(int state, float4 t0, float4 t1, V3 o)
{
    const float x = t0.x - o.x, y = t0.y - o.y, z = t0.z - o.z;
    const float n = x * t0.w + y * t1.x + z * t1.y;
    return state == kCullKeeps || (state == kCullAsk && !(n >= kCullMin));
}

constexpr int kViewFrameChunk = 8;
static_assert(kViewFrameChunk * kMaxViewInstances <= 256, "one thread per (frame of the chunk, instance) computes its origin");

__global__ __launch_bounds__(256) void view_records_kernel(const RenderParams p, const ViewJob job)
{
    __shared__ float origin[kViewFrameChunk * kMaxViewInstances][3];
    if (blockIdx.x >= job.record_blocks) {
        // one thread per lane of a tile: the lane's camera_space_direction, from the intrinsics every frame of the launch shares.
        // Lanes beyond a ragged edge write what they compute: the table has room for whole tiles and nothing reads those.
        const size_t k = ((size_t)blockIdx.y * job.dir_blocks + (blockIdx.x - job.record_blocks)) * 256 + threadIdx.x;
        const size_t tile = k >> 6, ntiles = (size_t)p.tiles_x * (size_t)p.tiles_y;
        if (tile >= ntiles) return;
        const int lane = (int)(k & 63);
        const int x = (int)(tile % (size_t)p.tiles_x) * kPrimTile + (lane & 7), y = (int)(tile / (size_t)p.tiles_x) * kPrimTile + (lane >> 3);   // pixel_of
        const V3 d = camera_space_direction(p.frames[0], (float)x, (float)y);
        float* out = const_cast<float*>(p.dir_table) + tile * (3 * 64) + lane;
        out[0] = d.x; out[64] = d.y; out[128] = d.z;
        return;
    }
    // the frames of this row of the grid, and their origins in every instance's mesh space
    const int frame0 = (int)blockIdx.y * kViewFrameChunk, frames = min(kViewFrameChunk, p.num_frames - frame0);
    if ((int)threadIdx.x < frames * job.n) {
        const FrameParams& f = p.frames[frame0 + (int)threadIdx.x / job.n];
        const V3 o = to_mesh_space(p.instances[(int)threadIdx.x % job.n], v3(f.origin[0], f.origin[1], f.origin[2]), v3(0.0f, 0.0f, 1.0f)).ro;
        origin[threadIdx.x][0] = o.x; origin[threadIdx.x][1] = o.y; origin[threadIdx.x][2] = o.z;
    }
    __syncthreads();
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    int rec = t >> 2;
    const int quarter = t & 3;
    char* view = (char*)p.records + p.view_base;
    if (rec >= job.total) {
        // the job.n threads behind the last record: the ray headers of the instance, one per frame, see RayHeader
        const int i = t - job.total * 4;
        if (i >= job.n) return;
        const DevInstance& in = p.instances[i];
        for (int k = 0; k < frames; k++) {
            const int frame = frame0 + k;
            const V3 o = v3(origin[k * job.n + i][0], origin[k * job.n + i][1], origin[k * job.n + i][2]);
            const float inf = __int_as_float(0x7f800000);
            const uint32_t flags = (fabsf(o.x) < inf && fabsf(o.y) < inf && fabsf(o.z) < inf ? kRayOriginFinite : 0u) |
                                   ((p.mesh_flags[in.mesh_index] & kBoxUnordered) != 0 ? kRayBoxUnordered : 0u) |
                                   (in.exact_uv != 0 ? kRayExactUv : 0u) | (in.unit_inv != 0 ? kRayUnitInv : 0u);
            const uint32_t vdelta = p.view_base + (uint32_t)frame * p.view_frame_stride + (uint32_t)p.view_inst_off[i];
            float4* h = (float4*)(view + (size_t)frame * p.view_frame_stride) + (size_t)i * 4;
            h[0] = make_float4(o.x, o.y, o.z, __uint_as_float(flags));
            h[1] = make_float4(in.q_rot.x, in.q_rot.y, in.q_rot.z, in.q_rot.w);
            h[2] = make_float4(in.inv_scale[0], in.inv_scale[1], in.inv_scale[2], __int_as_float(in.root_ref));
            h[3] = make_float4(in.inv_pose_xyz[0], in.inv_pose_xyz[1], in.inv_pose_xyz[2], __uint_as_float(vdelta));
        }
        return;
    }
    int i = 0;
    while (i + 1 < job.n && rec >= job.count[i]) { rec -= job.count[i]; i++; }
    const float4 w = p.records[(size_t)(job.node_base[i] + rec) * 4 + quarter];
    // The cull: the four threads of a record take one triangle each of either child, read here once for all frames.
    int state_a = kCullKeeps, state_b = kCullKeeps;
    float4 a0 = w, a1 = w, b0 = w, b1 = w;
    if (job.cull) {
        const float4 q3 = p.records[(size_t)(job.node_base[i] + rec) * 4 + 3];
        state_a = cull_triangle(p, job, __float_as_int(q3.x), quarter, a0, a1);
        state_b = cull_triangle(p, job, __float_as_int(q3.y), quarter, b0, b1);
    }
    float4* out = (float4*)view + (size_t)(job.first[i] + rec) * 4 + quarter;
    for (int k = 0; k < frames; k++) {
        const int frame = frame0 + k;
        const V3 o = v3(origin[k * job.n + i][0], origin[k * job.n + i][1], origin[k * job.n + i][2]);
        float4 v = w;
        if (quarter == 0) v = make_float4(w.x - o.x, w.y - o.y, w.z - o.z, w.w - o.x);          // the operand order of box_differences
        else if (quarter == 1) v = make_float4(w.x - o.y, w.y - o.z, w.z - o.x, w.w - o.y);
        else if (quarter == 2) v = make_float4(w.x - o.z, w.y - o.x, w.z - o.y, w.w - o.z);
        if (job.cull) {
            // A child none of whose triangles keeps it gets six NaN box words (kCullWord): every plane product is a NaN for any dinv,
            // min / max of NaNs stay NaN, and `far >= near` is false in the octant forms and in the generic slab test alike -- the
            // generic test sorts the two products of an axis, so +inf / -inf planes would PASS it.  (Wave-uniform control flow here:
            // the four threads of a record are neighbours of one wave, and every thread of the wave runs the same frames.)
            const unsigned long long ka = __ballot(cull_keeps(state_a, a0, a1, o));
            const unsigned long long kb = __ballot(cull_keeps(state_b, b0, b1, o));
            const int group = (int)(threadIdx.x & 60u);
            const bool dead_a = ((ka >> group) & 15ull) == 0ull, dead_b = ((kb >> group) & 15ull) == 0ull;
            const float dead = __int_as_float(kCullWord);
            if (quarter == 0) { if (dead_a) v = make_float4(dead, dead, dead, dead); }
            else if (quarter == 1) { if (dead_a) { v.x = dead; v.y = dead; } if (dead_b) { v.z = dead; v.w = dead; } }
            else if (quarter == 2) { if (dead_b) v = make_float4(dead, dead, dead, dead); }
        }
        *(float4*)((char*)out + (size_t)frame * p.view_frame_stride) = v;
    }
}

// rt_scene_view_cull_stats (diagnostics, never part of a render): the culled children in one instance's part of the views of one
// launch -- a leaf child of one to four coded triangles whose x planes are kCullWord, the NaN no box minus origin gives.
// One thread per view record, blockIdx.y = the frame.
__global__ __launch_bounds__(256) void view_cull_count_kernel(const float4* records, uint32_t view_base, uint32_t frame_stride, int32_t first,
                                                              int32_t count, unsigned long long* out)
{
    const int rec = (int)(blockIdx.x * 256 + threadIdx.x);
    if (rec >= count) return;
    const float4* q = (const float4*)((const char*)records + view_base + (size_t)blockIdx.y * frame_stride) + (size_t)(first + rec) * 4;
    const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const int pinf = kCullWord, ninf = kCullWord;
    auto coded_leaf = [](int32_t ref) { const int c = (ref >> kSlotBits) & 31; return ref < 0 && c >= 1 && c <= 4; };
    const int n = (coded_leaf(__float_as_int(q3.x)) && __float_as_int(q0.x) == pinf && __float_as_int(q0.w) == ninf ? 1 : 0) +
                  (coded_leaf(__float_as_int(q3.y)) && __float_as_int(q1.z) == pinf && __float_as_int(q2.y) == ninf ? 1 : 0);
    if (n) atomicAdd(&out[blockIdx.y], (unsigned long long)n);
}

// ---------------------------------------------------------------------------------------------------------
// Ray queries (rt_trace_rays / rt_occluded / rt_camera_rays): the reference's cast_ray (raycast.cu:21-142) on rays the caller
// chooses.  No new traversal: cast_ray_ex with per-lane origins (SEC: the hand-written loop when a wave's rays share a sign octant in
// mesh space, the compiler's loop on the general stack otherwise), one wave per workgroup like the primary kernels.  The scene's
// per-sample extension scratch is not touched: queries on one scene may overlap each other and renders on other streams.
// ---------------------------------------------------------------------------------------------------------
struct QueryParams {
    const float* org;           // [n][3] world origins
    const float* dir;           // [n][3] world directions (not normalised: cast_ray takes them as they are)
    const float* tmax;          // rt_occluded: [n] light distances, null = FLT_MAX
    const int32_t* order;       // octant binning: workgroup slot k traces ray order[k] (null = ray k)
    int32_t n;
    float* t;                   // outputs, each optional (null = not wanted), indexed by the ray's ORIGINAL index
    int32_t *instance, *triangle;
    float *location, *normal, *uv;
    int32_t* pops;
    uint8_t* occluded;
    int32_t* bins;              // octant binning: [0..7] rays per octant, [8..15] the scatter's cursors
};
constexpr int kQueryBlock = 64;
typedef StackT<kQueryBlock> QueryStack;

// the ray a workgroup slot traces (read again after the cast instead of being kept across it: registers the loop has no room for)
__device__ __forceinline__ int32_t query_ray(const QueryParams& q, int32_t slot) { return q.order ? q.order[slot] : slot; }

// ANYHIT = rt_occluded: cast_ray_lp(ray, lighting_pass = 1, light_distance = tmax[i]) (raycast.cu:129-133); occluded = the cast accepted a
// hit below tmax (= its min < tmax, except that a miss is not occluded when tmax is +inf).
// Otherwise rt_trace_rays: cast_ray(ray) and the fields of its HitInfo.  Rays with non-finite components run like any other ray
// (no usable octant: the compiler's generic loop); what they return is unspecified, other lanes' results are not affected.
template <bool ANYHIT>
__global__ __launch_bounds__(kQueryBlock, 8) void query_kernel(const RenderParams p, const QueryParams q)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth) + 1][kQueryBlock]
    const int32_t slot0 = (int32_t)blockIdx.x * kQueryBlock;    // (< n <= INT32_MAX: no overflow)
    if (slot0 + (int32_t)threadIdx.x >= q.n) return;
    int32_t i = query_ray(q, slot0 + (int32_t)threadIdx.x);
    const size_t i3 = (size_t)i * 3;
    const V3 org = v3(q.org[i3], q.org[i3 + 1], q.org[i3 + 2]);
    const V3 dir = v3(q.dir[i3], q.dir[i3 + 1], q.dir[i3 + 2]);
    const float tmax = (ANYHIT && q.tmax) ? q.tmax[i] : FLT_MAX;
    int spill[kMaxStack - kLdsStack];
    QueryStack stack;
    // (the thread's index lives on as the address of its LDS stack column only, as in render_ex_kernel)
    stack.lds = (lds_int*)lds_stack + threadIdx.x; stack.spill = spill; stack.lds_depth = lds_rows(p.stack_depth); stack.sp = 0;
    int pops = 0;
    const Hit hit = cast_ray_ex<!ANYHIT, true, ANYHIT, QueryStack, true, false, false, true>(p, org, dir, stack, pops, tmax);
    asm volatile("" : "+v"(stack.lds));
    i = query_ray(q, slot0 + (int32_t)(stack.lds - (lds_int*)lds_stack));
    if constexpr (ANYHIT) {
        q.occluded[i] = any_hit_done(hit, q.tmax ? q.tmax[i] : FLT_MAX) ? 1 : 0;
    } else {
        const bool got = hit.instance >= 0;
        if (q.t) q.t[i] = hit.min;
        if (q.instance) q.instance[i] = hit.instance;
        if (q.triangle) q.triangle[i] = got ? p.tri_id[hit.slot] : -1;
        if (q.pops) q.pops[i] = pops;
        const size_t o3 = (size_t)i * 3;
        if (q.location) { q.location[o3] = hit.loc.x; q.location[o3 + 1] = hit.loc.y; q.location[o3 + 2] = hit.loc.z; }
        if (q.normal) {
            const V3 n = got ? hit_normal(p, hit) : v3(0.0f, 0.0f, 0.0f);
            q.normal[o3] = n.x; q.normal[o3 + 1] = n.y; q.normal[o3 + 2] = n.z;
        }
        if (q.uv) {
            // TrianglePrimitive::point_inside's interpolated uv, as base_colour derives it (exact-uv meshes: the hit carries it)
            float2 uv = make_float2(0.0f, 0.0f);
            if (got) {
                uv = make_float2(hit.u, hit.v);
                if (!p.instances[hit.instance].exact_uv) {
                    const float* t = p.tri_uv + (size_t)hit.slot * 6;
                    const float w = 1.0f - hit.u - hit.v;
                    uv.x = (w * t[0] + hit.v * t[2]) + hit.u * t[4];
                    uv.y = (w * t[1] + hit.v * t[3]) + hit.u * t[5];
                }
            }
            q.uv[(size_t)i * 2] = uv.x; q.uv[(size_t)i * 2 + 1] = uv.y;
        }
    }
}

// Visibility masks (rt_visibility, include/rt_hip.h "visibility masks"): which of the caller's points see the
// surface a pixel's primary ray hit.  The rays are made HERE from the staged G-buffer planes: origin = the point L, direction =
// X - L (not normalised), bound = magnitude(X - L) * (1 - bias), cast as query_kernel<true> casts rt_occluded's rays -- the same
// cast_ray_ex instantiation, the same any_hit_done, so bit k is exactly `rt_occluded answers 0`.  One wave per workgroup, one 8x8
// tile of one frame per wave (workgroup (x, y, z) = tile (x, ty0 + y) of frame frame0 + z): a wave's rays share their origin, so they
// almost always share a sign octant and stay in the hand-written loop.  The frame's point is an expression of blockIdx and the loop
// counter, hence wave-uniform, and arrives by scalar loads (the address space says the words do not change while the kernel runs).
// A lane that is outside the frame or whose pixel is a miss leaves before the loop (the miss stores its zeros first), so a wave
// without a hit is gone at once and the loop's control stays uniform among the lanes that remain.  Across the cast a lane keeps its
// mask and the address of its LDS column; the pixel and X are derived from the column again for every point (query_kernel's way:
// registers the loop has no room for; the re-read is 12 bytes per lane from a line the cache holds).  `facing` needs no cast and has
// a loop of its own after the casts, so that only one mask is carried.  One int32 store per plane and pixel, no atomics, no zero fill.
struct VisParams {
    const int32_t* instance;    // staged planes [count][height][width](x3)
    const float* location;
    const float* normal;        // null unless facing
    const float* points;        // [count][num_points][3] world
    int32_t width, height, num_points;
    int32_t frame0, ty0;        // this launch's first frame and first tile row (a grid's y and z end at 65 535)
    float bias;
    int32_t *visible, *facing;  // [count][height][width], each optional
};
typedef const __attribute__((address_space(4))) float* VisPointPtr;

// the pixel of the lane whose LDS column is `column`, and its element in a frame-major plane; false = outside the frame
__device__ __forceinline__ bool visibility_pixel(const VisParams& v, const lds_int* column, const lds_int* base, size_t& px)
{
    const int lane = (int)(column - base);
    const int x = (int)blockIdx.x * kPrimTile + (lane & 7), y = (v.ty0 + (int)blockIdx.y) * kPrimTile + (lane >> 3);
    px = (((size_t)v.frame0 + blockIdx.z) * (size_t)v.height + (size_t)y) * (size_t)v.width + (size_t)x;
    return x < v.width && y < v.height;
}

__global__ __launch_bounds__(kQueryBlock, 8) void visibility_kernel(const RenderParams p, const VisParams v)
{
    static_assert(kQueryBlock == kPrimTile * kPrimTile, "one wave = one 8x8 tile");
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth) + 1][kQueryBlock]
    lds_int* column = (lds_int*)lds_stack + threadIdx.x;
    size_t px;
    if (!visibility_pixel(v, column, (lds_int*)lds_stack, px)) return;
    if (v.instance[px] < 0) {                                   // rule 8
        if (v.visible) v.visible[px] = 0;
        if (v.facing) v.facing[px] = 0;
        return;
    }
    const VisPointPtr pts = (VisPointPtr)(uintptr_t)(v.points + ((size_t)v.frame0 + blockIdx.z) * (size_t)v.num_points * 3);
    if (v.visible) {
        int spill[kMaxStack - kLdsStack];
        QueryStack stack;
        stack.lds = column; stack.spill = spill; stack.lds_depth = lds_rows(p.stack_depth);
        const float s = 1.0f - v.bias;                          // rule 3
        uint32_t mask = 0;
        for (int k = 0; k < v.num_points; k++) {
            asm volatile("" : "+v"(stack.lds));
            visibility_pixel(v, stack.lds, (lds_int*)lds_stack, px);
            const V3 L = v3(pts[k * 3], pts[k * 3 + 1], pts[k * 3 + 2]);
            const V3 d = v3(v.location[px * 3] - L.x, v.location[px * 3 + 1] - L.y, v.location[px * 3 + 2] - L.z);      // rule 1
            const float tmax = magnitude(d) * s;                // rules 2, 4
            stack.sp = 0;
            int pops = 0;
            const Hit hit = cast_ray_ex<false, true, true, QueryStack, true, false, false, true>(p, L, d, stack, pops, tmax);
            if (!any_hit_done(hit, tmax)) mask |= 1u << k;      // rule 5
        }
        asm volatile("" : "+v"(stack.lds));
        column = stack.lds;
        visibility_pixel(v, column, (lds_int*)lds_stack, px);
        v.visible[px] = (int32_t)mask;
    }
    if (v.facing) {
        const V3 X = v3(v.location[px * 3], v.location[px * 3 + 1], v.location[px * 3 + 2]);
        const V3 n = v3(v.normal[px * 3], v.normal[px * 3 + 1], v.normal[px * 3 + 2]);
        uint32_t mask = 0;
        for (int k = 0; k < v.num_points; k++) {
            const V3 w = v3(pts[k * 3] - X.x, pts[k * 3 + 1] - X.y, pts[k * 3 + 2] - X.z);      // rule 6
            if (n.x * w.x + n.y * w.y + n.z * w.z > 0.0f) mask |= 1u << k;                      // rule 7
        }
        v.facing[px] = (int32_t)mask;
    }
}

// Octant binning: a wave of arbitrary rays almost never shares a sign octant, and a wave that does not leaves the hand-written loop.
// The two passes below sort the ray indices by the sign octant of their WORLD direction (a counting sort of 8 buckets; rays of
// rotated instances may still differ in mesh space -- those waves fall back per instance, as they would unsorted).  Each workgroup
// takes a chunk of kBinChunk rays; per wave a ballot per bucket, one atomic per bucket per workgroup.  The order within a bucket
// depends on which workgroup reserves first -- only the order of the work, never what a ray computes.
constexpr int kBinBlock = 256, kBinChunk = 4096;
__device__ __forceinline__ int world_octant(const QueryParams& q, int32_t i)
{
    const size_t i3 = (size_t)i * 3;
    return (int)(__float_as_uint(q.dir[i3]) >> 31) | (int)((__float_as_uint(q.dir[i3 + 1]) >> 31) << 1) |
           (int)((__float_as_uint(q.dir[i3 + 2]) >> 31) << 2);
}

// this workgroup's rays per octant -> counts[8] (LDS); lane 0 of each wave adds its wave's popcounts
__device__ __forceinline__ void bin_chunk_counts(const QueryParams& q, int32_t first, int32_t last, int* counts)
{
    if (threadIdx.x < 8) counts[threadIdx.x] = 0;
    __syncthreads();
    int mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t k = first + (int32_t)threadIdx.x; k - (int32_t)threadIdx.x < last; k += kBinBlock) {
        const int oct = k < last ? world_octant(q, k) : -1;
        for (int b = 0; b < 8; b++) mine[b] += __popcll(__ballot(oct == b));
    }
    if ((threadIdx.x & 63) == 0)
        for (int b = 0; b < 8; b++) if (mine[b]) atomicAdd(&counts[b], mine[b]);
    __syncthreads();
}

__global__ __launch_bounds__(kBinBlock) void bin_count_kernel(const QueryParams q)
{
    __shared__ int counts[8];
    const int32_t first = (int32_t)((int64_t)blockIdx.x * kBinChunk), last = (int32_t)std::min<int64_t>((int64_t)first + kBinChunk, q.n);
    bin_chunk_counts(q, first, last, counts);
    if (threadIdx.x < 8 && counts[threadIdx.x]) atomicAdd(&q.bins[threadIdx.x], counts[threadIdx.x]);
}

__global__ __launch_bounds__(kBinBlock) void bin_scatter_kernel(const QueryParams q, int32_t* order)
{
    __shared__ int counts[8], base[8], wave_counts[kBinBlock / 64][8];
    const int32_t first = (int32_t)((int64_t)blockIdx.x * kBinChunk), last = (int32_t)std::min<int64_t>((int64_t)first + kBinChunk, q.n);
    bin_chunk_counts(q, first, last, counts);
    if (threadIdx.x < 8) {
        int start = 0;                                          // the bucket's first index: the rays of the octants before it
        for (int b = 0; b < (int)threadIdx.x; b++) start += q.bins[b];
        base[threadIdx.x] = start + (counts[threadIdx.x] ? atomicAdd(&q.bins[8 + threadIdx.x], counts[threadIdx.x]) : 0);
    }
    __syncthreads();
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int32_t k0 = first; k0 < last; k0 += kBinBlock) {
        const int32_t k = k0 + (int32_t)threadIdx.x;
        const int oct = k < last ? world_octant(q, k) : -1;
        int rank = 0;
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot(oct == b);
            if (lane == 0) wave_counts[wave][b] = __popcll(m);
            if (oct == b) rank = __popcll(m & below);
        }
        __syncthreads();
        if (oct >= 0) {
            int at = base[oct] + rank;
            for (int w = 0; w < wave; w++) at += wave_counts[w][oct];
            order[at] = k;
        }
        __syncthreads();
        if (threadIdx.x < 8) {
            int add = 0;
            for (int w = 0; w < kBinBlock / 64; w++) add += wave_counts[w][threadIdx.x];
            base[threadIdx.x] += add;
        }
        __syncthreads();
    }
}

// rt_camera_rays: the primary ray of every pixel, exactly as render_pixel makes it (raycast.cu:156-188), row-major y * width + x
__global__ __launch_bounds__(256) void camera_rays_kernel(const FrameParams f, int32_t width, size_t npix, float* org, float* dir)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= npix) return;
    const int x = (int)(k % (size_t)width), y = (int)(k / (size_t)width);
    const V3 d = world_direction(f, camera_space_direction(f, (float)x, (float)y));
    org[k * 3] = f.origin[0]; org[k * 3 + 1] = f.origin[1]; org[k * 3 + 2] = f.origin[2];
    dir[k * 3] = d.x; dir[k * 3 + 1] = d.y; dir[k * 3 + 2] = d.z;
}

// rt_camera_directions: camera_space_direction of every pixel, row-major -- what the view pre-pass fills a launch's table with
__global__ __launch_bounds__(256) void camera_directions_kernel(const FrameParams f, int32_t width, size_t npix, float* dir)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= npix) return;
    const int x = (int)(k % (size_t)width), y = (int)(k / (size_t)width);
    const V3 d = camera_space_direction(f, (float)x, (float)y);
    dir[k * 3] = d.x; dir[k * 3 + 1] = d.y; dir[k * 3 + 2] = d.z;
}

// rt_ray_table_create: the caller's row-major directions [height][width][3] into the tiled layout render_pixel<.., TABLE> reads
// (tile ty * tiles_x + tx = 3 x 64 words, x / y / z planes 64 apart, lane (y & 7) * 8 + (x & 7)).  One thread per WORD OF THE TABLE,
// in table order: a wave writes 256 consecutive bytes; the reads are the strided side (eight runs of eight pixels, 12 bytes apart).
// The words are moved as integers: the table holds the caller's bits, whatever they are.  Lanes beyond a ragged edge get (0, 1, 0).
__global__ __launch_bounds__(256) void ray_table_pack_kernel(const uint32_t* src, int32_t width, int32_t height, int32_t tiles_x, size_t nwords,
                                                             uint32_t* table)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nwords) return;
    const size_t tile = k / (3 * 64);
    const int r = (int)(k % (3 * 64)), plane = r >> 6, lane = r & 63;
    const int x = (int)(tile % (size_t)tiles_x) * kPrimTile + (lane & 7), y = (int)(tile / (size_t)tiles_x) * kPrimTile + (lane >> 3);
    uint32_t w = plane == 1 ? 0x3f800000u : 0u;
    if (x < width && y < height) w = src[((size_t)y * (size_t)width + (size_t)x) * 3 + (size_t)plane];
    table[k] = w;
}

// rt_ray_table_rays: rt_camera_rays for a table -- world_direction of the entry, the frame's origin; row-major y * width + x
__global__ __launch_bounds__(256) void ray_table_rays_kernel(const FrameParams f, const float* table, int32_t width, int32_t tiles_x, size_t npix,
                                                             float* org, float* dir)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= npix) return;
    const int x = (int)(k % (size_t)width), y = (int)(k / (size_t)width);
    const float* t = table + ((size_t)(y / kPrimTile) * (size_t)tiles_x + (size_t)(x / kPrimTile)) * (3 * 64) + (size_t)((y & 7) * 8 + (x & 7));
    const V3 d = world_direction(f, v3(t[0], t[64], t[128]));
    org[k * 3] = f.origin[0]; org[k * 3 + 1] = f.origin[1]; org[k * 3 + 2] = f.origin[2];
    dir[k * 3] = d.x; dir[k * 3 + 1] = d.y; dir[k * 3 + 2] = d.z;
}

// ---------------------------------------------------------------------------------------------------------
// Closest-point queries (rt_closest_points): the nearest point of the scene's triangles to each of the caller's points, equal bit for
// bit to a brute-force minimum over every (instance, triangle) -- the rule is in include/rt_hip.h, the pruning argument in DESIGN.md
// section 11.  One wave per workgroup, one point per lane, a nearest-first traversal of each instance's tree on the general stack.
// ---------------------------------------------------------------------------------------------------------
struct PointParams {
    const float4* records;
    const float* tri_uv;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* pts;           // [n][3] world points
    const float* max_distance;  // [n] or null (= +inf)
    int32_t n;
    float* distance;            // outputs, each optional (null = not wanted)
    int32_t *instance, *triangle;
    float *point, *normal, *barycentric, *uv;
    int32_t* pops;
};
constexpr int kPointBlock = 64;
typedef StackT<kPointBlock> PointStack;

// What the one-wave query kernels (kPointBlock, kCrossBlock, kTriBlock: one query per lane) share.
// A lane's stack: its column of the workgroup's LDS block and the overflow array its kernel declares
__device__ __forceinline__ StackT<64> query_stack(int* lds_stack, int* spill, int stack_depth)
{
    StackT<64> stack;
    stack.lds = (lds_int*)lds_stack + threadIdx.x; stack.spill = spill; stack.lds_depth = lds_rows(stack_depth); stack.sp = 0;
    return stack;
}

// The unordered traversal of instance in's tree, for the queries that want every pair and no order: crossings, crossing lists and
// sections (ti_trace, bx_trace and rg_trace keep this loop written out: on the walker one intersect kernel spills two more registers
// and the long box and region lists measured under 1 % slower).
// box(lx, ly, lz, hx, hy, hz) says whether a child box may hold a pair; it is asked only where `prune` (the caller clears it for a
// mesh with unordered / NaN boxes: no pruning in this mesh), child a and then child b, and b is postponed when both pass.
// leaf(slot, t0, t1, t2) gets one triangle's record, triangles in tree order, and returns whether to end the traversal.  pops counts
// the interior nodes visited.  Returns whether leaf ended it.  P: any query's params.
template <typename P, typename Box, typename Leaf>
__device__ __forceinline__ bool walk_unordered(const P& p, StackT<64>& stack, const DevInstance& in, bool prune, int32_t& pops, Box&& box,
                                               Leaf&& leaf)
{
    bool done = false;
    stack.sp = 0;
    stack.push(kSentinel);
    int32_t cur = in.root_ref, rem = -1;
    do {
        if (cur >= 0) {                                         // interior node: every child that passes, no order
            pops++;
            const float4* rec = p.records + (size_t)cur * 4;
            const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
            const bool pa = !prune || box(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y);
            const bool pb = !prune || box(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w);
            const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
            if (pa && pb) stack.push(rb);
            cur = pa ? ra : (pb ? rb : kNeedPop);
        } else {                                                // one triangle of a leaf per iteration
            const int32_t slot = cur & kSlotMask;
            if (rem < 0) {
                rem = (cur >> kSlotBits) & 31;
                if (rem == 31) rem = p.leaf_count[slot];        // (leaves of more than 30 triangles)
            }
            if (rem > 0) {
                const float4* rec = p.records + (size_t)slot * 4;
                if (leaf(slot, rec[0], rec[1], rec[2])) done = true;
            }
            rem--;
            cur = rem > 0 ? cur + 1 : kNeedPop;
            rem = rem > 0 ? rem : -1;
        }
        if (cur == kNeedPop) cur = stack.pop();
    } while (cur != kSentinel && !done);
    return done;
}
template <typename P>
__device__ __forceinline__ bool boxes_ordered(const P& p, const DevInstance& in) { return (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0; }

// A list room kept as a lane-private max-heap of its entries' keys while pairs arrive, and sorted in place at the end: a pair enters
// in O(log room).  A: the room's accessor, get(q) and put(q, item) on absolute slots; an item has .key, and whatever travels with it.
// (instance, triangle) as one key, compared as a pair (both >= 0 in a filled slot)
__device__ __forceinline__ uint64_t pair_key(int32_t instance, int32_t triangle) { return ((uint64_t)(uint32_t)instance << 32) | (uint64_t)(uint32_t)triangle; }
// `it` enters the heap of `size` slots at `start` from slot `pos` downwards: greater children move up until it fits
template <typename A, typename Item>
__device__ __forceinline__ void room_sift_down(const A& a, size_t start, uint64_t size, uint64_t pos, Item it)
{
    for (;;) {
        uint64_t child = 2 * pos + 1;
        if (child >= size) break;
        Item ci = a.get(start + (size_t)child);
        if (child + 1 < size) {
            const Item c2 = a.get(start + (size_t)child + 1);
            if (c2.key > ci.key) { ci = c2; child++; }
        }
        if (ci.key <= it.key) break;
        a.put(start + (size_t)pos, ci);
        pos = child;
    }
    a.put(start + (size_t)pos, it);
}
// One pair arrives: while the room fills it sifts up from the new last slot; a full room takes it only below its greatest key, the
// root, which leaves.  Which keys stay does not depend on the order of arrival.
template <typename A, typename Item>
__device__ __forceinline__ void room_insert(const A& a, size_t start, uint64_t room, uint64_t& filled, Item it)
{
    if (filled < room) {
        uint64_t pos = filled++;
        while (pos > 0) {
            const uint64_t parent = (pos - 1) / 2;
            const Item pi = a.get(start + (size_t)parent);
            if (pi.key >= it.key) break;
            a.put(start + (size_t)pos, pi);
            pos = parent;
        }
        a.put(start + (size_t)pos, it);
    } else if (it.key < a.get(start).key) {
        room_sift_down(a, start, room, 0, it);
    }
}
// heap -> ascending: the greatest key to the end, the rest a heap again
template <typename A>
__device__ __forceinline__ void room_sort(const A& a, size_t start, uint64_t filled)
{
    for (uint64_t end = filled; end > 1; end--) {
        const auto last = a.get(start + (size_t)(end - 1));
        a.put(start + (size_t)(end - 1), a.get(start));
        room_sift_down(a, start, end - 1, 0, last);
    }
}

// Ericson's closest point on triangle (A, A + AB, A + AC) to q (Real-Time Collision Detection 5.1.5), returned as the weights (b1, b2) of
// AB and AC, in one fixed fp32 sequence.  An edge ratio whose denominator is not > 0 is 0 (and a ratio is never above 1).  Where the
// classification reaches the face region with a negative va, vb or vc or a sum that is not > 0 (rounding on nearly degenerate
// triangles; NaN input), the weights are those of the nearest of the three edges AB, AC, BC instead (first of equals in that order),
// each the clamped projection onto its segment.  The weights are always finite, in [0, 1], and b1 + b2 <= 1 up to rounding.
__device__ __forceinline__ float pq_ratio(float a, float b) { return b > 0.0f ? fminf(a / b, 1.0f) : 0.0f; }
__device__ __forceinline__ float pq_d2(V3 d) { return (d.x * d.x + d.y * d.y) + d.z * d.z; }
__device__ __forceinline__ V3 pq_combine(V3 a, V3 ab, V3 ac, float b1, float b2)
{
    return v3((a.x + b1 * ab.x) + b2 * ac.x, (a.y + b1 * ab.y) + b2 * ac.y, (a.z + b1 * ab.z) + b2 * ac.z);
}
// the clamped projection of q onto the segment p0 + t * d, t in [0, 1] (0 for a zero-length d)
__device__ __forceinline__ float pq_segment(V3 q, V3 p0, V3 d)
{
    const float dd = dot(d, d);
    const float t = dd > 0.0f ? dot(q - p0, d) / dd : 0.0f;
    return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;         // (a NaN t gives 0)
}
__device__ __noinline__ float2 pq_fallback(V3 q, V3 a, V3 ab, V3 ac)
{
    const float t0 = pq_segment(q, a, ab), t1 = pq_segment(q, a, ac), t2 = pq_segment(q, a + ab, ac - ab);
    float2 w = make_float2(t0, 0.0f);
    float best = pq_d2(q - pq_combine(a, ab, ac, t0, 0.0f));
    const float e1 = pq_d2(q - pq_combine(a, ab, ac, 0.0f, t1));
    if (e1 < best) { best = e1; w = make_float2(0.0f, t1); }
    const float s = 1.0f - t2;
    const float e2 = pq_d2(q - pq_combine(a, ab, ac, s, t2));
    if (e2 < best) w = make_float2(s, t2);
    return w;
}
__device__ __forceinline__ float2 pq_weights(V3 q, V3 a, V3 ab, V3 ac)
{
    const V3 ap = q - a;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) return make_float2(0.0f, 0.0f);                          // vertex A
    const V3 bp = ap - ab;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) return make_float2(1.0f, 0.0f);                            // vertex B
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) return make_float2(pq_ratio(d1, d1 - d3), 0.0f);         // edge AB
    const V3 cp = ap - ac;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) return make_float2(0.0f, 1.0f);                            // vertex C
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) return make_float2(0.0f, pq_ratio(d2, d2 - d6));         // edge AC
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {                                        // edge BC
        const float w = pq_ratio(e43, e43 + e56);
        return make_float2(1.0f - w, w);
    }
    const float sum = (va + vb) + vc;
    if (va >= 0.0f && vb >= 0.0f && vc >= 0.0f && sum > 0.0f) {                             // face
        return make_float2(vb / sum, vc / sum);                                             // (each <= 1: vb, vc <= sum)
    }
    return pq_fallback(q, a, ab, ac);
}

// A triangle record's (A, AB, AC) in scaled mesh space: v0, e1 = v1 - v0 and e0 = v2 - v0 as stored, times the instance's scale
__device__ __forceinline__ void pq_triangle(float4 t0, float4 t1, float4 t2, V3 s, V3& a, V3& ab, V3& ac)
{
    a = v3(t0.x * s.x, t0.y * s.y, t0.z * s.z);
    ab = v3(t2.y * s.x, t2.z * s.y, t2.w * s.z);
    ac = v3(t1.z * s.x, t1.w * s.y, t2.x * s.z);
}

// A lower bound of d2 (the same fp32 sum of squares) for every triangle whose vertices lie in the mesh-space box lo..hi (DESIGN.md
// section 11): the box is scaled (a negative scale swaps the ends), widened by 2^-16 of its largest coordinate magnitude plus FLT_MIN,
// and the gap per axis is taken only where a compare says it is positive, so a NaN anywhere gives 0 on that axis, never a prune.
__device__ __forceinline__ float pq_gap(float lo, float hi, float s, float q)
{
    const float x = lo * s, y = hi * s;
    const float l = s < 0.0f ? y : x, h = s < 0.0f ? x : y;
    const float m = fmaxf(fabsf(l), fabsf(h)) * 0x1p-16f + 0x1p-126f;
    const float a = (l - m) - q, b = q - (h + m);
    return a > 0.0f ? a : (b > 0.0f ? b : 0.0f);
}
__device__ __forceinline__ float pq_box_lb(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, V3 q)
{
    const float gx = pq_gap(lx, hx, s.x, q.x), gy = pq_gap(ly, hy, s.y, q.y), gz = pq_gap(lz, hz, s.z, q.z);
    return (gx * gx + gy * gy) + gz * gz;
}

// The candidate bound in d2: the largest float x with sqrtf(x) <= max_distance (sqrtf is monotone, so sqrtf(d2) <= max_distance exactly
// when d2 <= x), found by bisection over the bit patterns of [0, +inf]; -1 when no d2 passes (NaN or negative bound).
__device__ __forceinline__ float pq_cut2(float maxd)
{
    if (!(0.0f <= maxd)) return -1.0f;                          // (sqrtf(0) = 0; -0 counts as 0)
    const float inf = __int_as_float(0x7f800000);
    if (sqrtf(inf) <= maxd) return inf;
    uint32_t lo = 0u, hi = 0x7f800000u;                         // sqrtf(lo) <= maxd < sqrtf(hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (sqrtf(__uint_as_float(mid)) <= maxd) lo = mid; else hi = mid;
    }
    return __uint_as_float(lo);
}

// world normal of triangle `slot` of instance `in`, as hit_normal gives it (raycast.cu:115-122); P: PointParams or NearbyParams
template <typename P>
__device__ __forceinline__ V3 pq_normal(const P& p, const DevInstance& in, int32_t slot)
{
    const float4* t = p.records + (size_t)slot * 4;
    const float4 t0 = t[0], t1 = t[1];
    V3 n = apply_quat(in.q_inv_rot, v3(t0.w, t1.x, t1.y));
    n.x *= in.scale[0]; n.y *= in.scale[1]; n.z *= in.scale[2];
    return normalize(n);
}

__global__ __launch_bounds__(kPointBlock, 8) void closest_point_kernel(const PointParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kPointBlock]
    const int32_t i = (int32_t)blockIdx.x * kPointBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const size_t i3 = (size_t)i * 3;
    const V3 w = v3(p.pts[i3], p.pts[i3 + 1], p.pts[i3 + 2]);
    const float cut2 = pq_cut2(p.max_distance ? p.max_distance[i] : __int_as_float(0x7f800000));
    int spill[kMaxStack - kLdsStack];
    PointStack stack = query_stack(lds_stack, spill, p.stack_depth);
    // the best candidate so far by (d2, instance, tri_id); best_inst < 0 = none yet
    float best = 0.0f, b1 = 0.0f, b2 = 0.0f;
    int32_t best_inst = -1, best_slot = 0, best_tid = 0, pops = 0;
    for (int32_t k = 0; k < p.num_instances && cut2 >= 0.0f; k++) {
        const DevInstance& in = p.instances[k];
        // the query point in scaled mesh space: to_mesh_space's origin before its inv_scale multiply
        const V3 q = apply_quat(in.q_pose, v3(w.x - in.pose_xyz[0], w.y - in.pose_xyz[1], w.z - in.pose_xyz[2]));
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: both child boxes, nearer first
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const float la = pq_box_lb(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, q);
                const float lb = pq_box_lb(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, q);
                const float lim = best_inst >= 0 ? best : cut2;
                const bool pa = !(prune && la > lim), pb = !(prune && lb > lim);
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                const bool a_near = !(lb < la);
                if (pa && pb) stack.push(a_near ? rb : ra);
                cur = (pa && pb) ? (a_near ? ra : rb) : (pa ? ra : (pb ? rb : kNeedPop));
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    const float4 t0 = rec[0], t1 = rec[1], t2 = rec[2];
                    V3 a, ab, ac;
                    pq_triangle(t0, t1, t2, s, a, ab, ac);
                    const float2 bw = pq_weights(q, a, ab, ac);
                    const float d2 = pq_d2(q - pq_combine(a, ab, ac, bw.x, bw.y));
                    if (d2 <= (best_inst >= 0 ? best : cut2)) {     // (NaN fails)
                        const int32_t tid = p.tri_id[slot];
                        if (best_inst < 0 || d2 < best || (best_inst == k && tid < best_tid)) {
                            best = d2; b1 = bw.x; b2 = bw.y; best_inst = k; best_slot = slot; best_tid = tid;
                        }
                    }
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel);
    }
    const bool got = best_inst >= 0;
    if (p.distance) p.distance[i] = got ? sqrtf(best) : FLT_MAX;
    if (p.instance) p.instance[i] = got ? best_inst : -1;
    if (p.triangle) p.triangle[i] = got ? best_tid : -1;
    if (p.pops) p.pops[i] = pops;
    if (p.barycentric) { p.barycentric[(size_t)i * 2] = got ? b1 : 0.0f; p.barycentric[(size_t)i * 2 + 1] = got ? b2 : 0.0f; }
    if (!got) {
        if (p.point) { p.point[i3] = 0.0f; p.point[i3 + 1] = 0.0f; p.point[i3 + 2] = 0.0f; }
        if (p.normal) { p.normal[i3] = 0.0f; p.normal[i3 + 1] = 0.0f; p.normal[i3 + 2] = 0.0f; }
        if (p.uv) { p.uv[(size_t)i * 2] = 0.0f; p.uv[(size_t)i * 2 + 1] = 0.0f; }
        return;
    }
    const DevInstance& in = p.instances[best_inst];
    if (p.point) {                                              // the winner's point again (same sequence), to world: apply_lre(inv_pose, c)
        const float4* rec = p.records + (size_t)best_slot * 4;
        V3 a, ab, ac;
        pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
        const V3 c = pq_combine(a, ab, ac, b1, b2);
        const V3 o = apply_quat(in.q_inv_pose, v3(c.x - in.inv_pose_xyz[0], c.y - in.inv_pose_xyz[1], c.z - in.inv_pose_xyz[2]));
        p.point[i3] = o.x; p.point[i3 + 1] = o.y; p.point[i3 + 2] = o.z;
    }
    if (p.normal) {
        const V3 n = pq_normal(p, in, best_slot);
        p.normal[i3] = n.x; p.normal[i3 + 1] = n.y; p.normal[i3 + 2] = n.z;
    }
    if (p.uv) {                                                 // w = (1 - b2) - b1, uv = (w uv0 + b1 uv1) + b2 uv2 (base_colour's order)
        const float* t = p.tri_uv + (size_t)best_slot * 6;
        const float u0 = (1.0f - b2) - b1;
        p.uv[(size_t)i * 2] = (u0 * t[0] + b1 * t[2]) + b2 * t[4];
        p.uv[(size_t)i * 2 + 1] = (u0 * t[1] + b1 * t[3]) + b2 * t[5];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Segment queries (rt_closest_to_segments): the nearest point of the scene's triangles to each of the caller's segments, equal bit for
// bit to a brute-force minimum over every (instance, triangle) -- rule 13 of include/rt_hip.h, the pruning argument in DESIGN.md
// section 18.  closest_point_kernel's shape: one wave per workgroup, one segment per lane, the nearest-first traversal, the lower
// bound now between the segment's box and the child's.  The crossing half (step 6) is segment_crossing_kernel, after xq_trace.
// ---------------------------------------------------------------------------------------------------------
struct SegParams {
    const float4* records;
    const float* tri_uv;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* segs;          // [n][2][3] world end points
    const float* max_distance;  // [n] or null (= +inf)
    int32_t n;
    float* distance;            // outputs, each optional (null = not wanted)
    int32_t *instance, *triangle;
    float *parameter, *segment_point, *point, *normal, *barycentric, *uv;
    int32_t* crossings;         // written by segment_crossing_kernel
    float* clearance;           // the distance here, set to 0 by segment_crossing_kernel where the segment crosses
    int32_t* within;            // 1 where there is a candidate here, set to 1 by segment_crossing_kernel where the segment crosses
    int32_t* pops;
};

__device__ __forceinline__ float sq_clamp01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }    // (a NaN gives 0)

// Ericson's closest pair of the segments q0 + s * d and e0 + u * f (Real-Time Collision Detection 5.1.9) as (s, u), both in [0, 1],
// in rule 13 step 4's fixed fp32 sequence (out of line: called three times per triangle)
__device__ __noinline__ float2 sq_segseg(V3 q0, V3 d, V3 e0, V3 f)
{
    const V3 r = q0 - e0;
    const float a = dot(d, d), e = dot(f, f), ff = dot(f, r);
    if (!(a > 0.0f)) return make_float2(0.0f, e > 0.0f ? sq_clamp01(ff / e) : 0.0f);
    const float c = dot(d, r);
    if (!(e > 0.0f)) return make_float2(sq_clamp01(-c / a), 0.0f);
    const float b = dot(d, f), den = a * e - b * b;
    float s = den > 0.0f ? sq_clamp01((b * ff - c * e) / den) : 0.0f;
    float u = (b * s + ff) / e;
    if (!(u >= 0.0f)) { u = 0.0f; s = sq_clamp01(-c / a); }
    else if (u > 1.0f) { u = 1.0f; s = sq_clamp01((b - c) / a); }
    return make_float2(s, u);
}

// One candidate (s, b1, b2) of a triangle against the best of the triangle so far (w = d2, x = s, y = b1, z = b2): the smaller d2,
// the earlier of equals; a NaN d2 never replaces one that is not NaN
__device__ __forceinline__ void sq_candidate(float4& best, V3 q0, V3 d, V3 a, V3 ab, V3 ac, float s, float b1, float b2)
{
    const V3 x = v3(q0.x + s * d.x, q0.y + s * d.y, q0.z + s * d.z);
    const float d2 = pq_d2(x - pq_combine(a, ab, ac, b1, b2));
    if (d2 < best.w || best.w != best.w) best = make_float4(s, b1, b2, d2);
}

// rule 13 step 3 on one triangle: (s, b1, b2, d2) of its candidate
__device__ __forceinline__ float4 sq_triangle(V3 q0, V3 q1, V3 a, V3 ab, V3 ac)
{
    const V3 d = q1 - q0;
    float4 best = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0x7fc00000));
    const float2 w0 = pq_weights(q0, a, ab, ac);
    sq_candidate(best, q0, d, a, ab, ac, 0.0f, w0.x, w0.y);
    const float2 w1 = pq_weights(q1, a, ab, ac);
    sq_candidate(best, q0, d, a, ab, ac, 1.0f, w1.x, w1.y);
    if (dot(d, d) > 0.0f) {                                     // (a zero-length segment is a point: closest_point_kernel's answer)
        const float2 e0 = sq_segseg(q0, d, a, ab);
        sq_candidate(best, q0, d, a, ab, ac, e0.x, e0.y, 0.0f);
        const float2 e1 = sq_segseg(q0, d, a, ac);
        sq_candidate(best, q0, d, a, ab, ac, e1.x, 0.0f, e1.y);
        const float2 e2 = sq_segseg(q0, d, a + ab, ac - ab);
        sq_candidate(best, q0, d, a, ab, ac, e2.x, 1.0f - e2.y, e2.y);
    }
    return best;
}

// One axis of the lower bound: the child's interval lo..hi scaled and widened exactly as pq_gap does it, against the segment's
// widened interval slo..shi; the gap only where a compare says it is positive (a NaN anywhere gives 0, never a prune)
__device__ __forceinline__ float sq_gap(float lo, float hi, float s, float slo, float shi)
{
    const float x = lo * s, y = hi * s;
    const float l = s < 0.0f ? y : x, h = s < 0.0f ? x : y;
    const float m = fmaxf(fabsf(l), fabsf(h)) * 0x1p-16f + 0x1p-126f;
    const float a = (l - m) - shi, b = slo - (h + m);
    return a > 0.0f ? a : (b > 0.0f ? b : 0.0f);
}
__device__ __forceinline__ float sq_box_lb(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, V3 slo, V3 shi)
{
    const float gx = sq_gap(lx, hx, s.x, slo.x, shi.x), gy = sq_gap(ly, hy, s.y, slo.y, shi.y), gz = sq_gap(lz, hz, s.z, slo.z, shi.z);
    return (gx * gx + gy * gy) + gz * gz;
}
// the segment's interval on one axis, widened by 2^-16 of its larger end magnitude plus FLT_MIN: every computed X of rule 13 lies in it
__device__ __forceinline__ void sq_interval(float a, float b, float& lo, float& hi)
{
    const float m = fmaxf(fabsf(a), fabsf(b)) * 0x1p-16f + 0x1p-126f;
    lo = fminf(a, b) - m; hi = fmaxf(a, b) + m;
}

// segment i's ends in instance `in`'s scaled mesh space (read again wherever they are needed: not held across the traversal)
__device__ __forceinline__ void sq_ends(const SegParams& p, int32_t i, const DevInstance& in, V3& q0, V3& q1)
{
    const float* g = p.segs + (size_t)i * 6;
    q0 = apply_quat(in.q_pose, v3(g[0] - in.pose_xyz[0], g[1] - in.pose_xyz[1], g[2] - in.pose_xyz[2]));
    q1 = apply_quat(in.q_pose, v3(g[3] - in.pose_xyz[0], g[4] - in.pose_xyz[1], g[5] - in.pose_xyz[2]));
}

// ANY: only within and / or pops are wanted of this half: the traversal ends at the first candidate, across instances too
template <bool ANY>
__global__ __launch_bounds__(kPointBlock, 8) void segment_closest_kernel(const SegParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kPointBlock]
    const int32_t i = (int32_t)blockIdx.x * kPointBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const size_t i3 = (size_t)i * 3;
    const float cut2 = pq_cut2(p.max_distance ? p.max_distance[i] : __int_as_float(0x7f800000));
    int spill[kMaxStack - kLdsStack];
    PointStack stack = query_stack(lds_stack, spill, p.stack_depth);
    // the best candidate so far by (d2, instance, tri_id); best_inst < 0 = none yet
    float best = 0.0f, bs = 0.0f, b1 = 0.0f, b2 = 0.0f;
    int32_t best_inst = -1, best_slot = 0, best_tid = 0, pops = 0;
    for (int32_t k = 0; k < p.num_instances && cut2 >= 0.0f && !(ANY && best_inst >= 0); k++) {
        const DevInstance& in = p.instances[k];
        V3 q0, q1, slo, shi;
        sq_ends(p, i, in, q0, q1);
        sq_interval(q0.x, q1.x, slo.x, shi.x); sq_interval(q0.y, q1.y, slo.y, shi.y); sq_interval(q0.z, q1.z, slo.z, shi.z);
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: both child boxes, nearer first
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const float la = sq_box_lb(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, slo, shi);
                const float lb = sq_box_lb(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, slo, shi);
                const float lim = best_inst >= 0 ? best : cut2;
                const bool pa = !(prune && la > lim), pb = !(prune && lb > lim);
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                const bool a_near = !(lb < la);
                if (pa && pb) stack.push(a_near ? rb : ra);
                cur = (pa && pb) ? (a_near ? ra : rb) : (pa ? ra : (pb ? rb : kNeedPop));
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                bool found = false;
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    const float4 t0 = rec[0], t1 = rec[1], t2 = rec[2];
                    V3 a, ab, ac;
                    pq_triangle(t0, t1, t2, s, a, ab, ac);
                    const float4 c = sq_triangle(q0, q1, a, ab, ac);
                    if (c.w <= (best_inst >= 0 ? best : cut2)) {    // (NaN fails)
                        const int32_t tid = p.tri_id[slot];
                        if (best_inst < 0 || c.w < best || (best_inst == k && tid < best_tid)) {
                            best = c.w; bs = c.x; b1 = c.y; b2 = c.z; best_inst = k; best_slot = slot; best_tid = tid;
                        }
                        found = true;
                    }
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
                if (ANY && found) break;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel);
    }
    const bool got = best_inst >= 0;
    if (p.pops) p.pops[i] = pops;
    if (p.within) p.within[i] = got ? 1 : 0;
    if constexpr (ANY) return;
    const float dist = got ? sqrtf(best) : FLT_MAX;
    if (p.distance) p.distance[i] = dist;
    if (p.clearance) p.clearance[i] = dist;
    if (p.instance) p.instance[i] = got ? best_inst : -1;
    if (p.triangle) p.triangle[i] = got ? best_tid : -1;
    if (p.parameter) p.parameter[i] = got ? bs : 0.0f;
    if (p.barycentric) { p.barycentric[(size_t)i * 2] = got ? b1 : 0.0f; p.barycentric[(size_t)i * 2 + 1] = got ? b2 : 0.0f; }
    if (!got) {
        if (p.segment_point) { p.segment_point[i3] = 0.0f; p.segment_point[i3 + 1] = 0.0f; p.segment_point[i3 + 2] = 0.0f; }
        if (p.point) { p.point[i3] = 0.0f; p.point[i3 + 1] = 0.0f; p.point[i3 + 2] = 0.0f; }
        if (p.normal) { p.normal[i3] = 0.0f; p.normal[i3 + 1] = 0.0f; p.normal[i3 + 2] = 0.0f; }
        if (p.uv) { p.uv[(size_t)i * 2] = 0.0f; p.uv[(size_t)i * 2 + 1] = 0.0f; }
        return;
    }
    const DevInstance& in = p.instances[best_inst];
    if (p.segment_point) {                                      // the winner's X again (same sequence), to world: apply_lre(inv_pose, X)
        V3 q0, q1;
        sq_ends(p, i, in, q0, q1);
        const V3 d = q1 - q0;
        const V3 x = v3(q0.x + bs * d.x, q0.y + bs * d.y, q0.z + bs * d.z);
        const V3 o = apply_quat(in.q_inv_pose, v3(x.x - in.inv_pose_xyz[0], x.y - in.inv_pose_xyz[1], x.z - in.inv_pose_xyz[2]));
        p.segment_point[i3] = o.x; p.segment_point[i3 + 1] = o.y; p.segment_point[i3 + 2] = o.z;
    }
    if (p.point) {                                              // the winner's c again (same sequence), closest_point_kernel's map
        const float4* rec = p.records + (size_t)best_slot * 4;
        V3 a, ab, ac;
        pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
        const V3 c = pq_combine(a, ab, ac, b1, b2);
        const V3 o = apply_quat(in.q_inv_pose, v3(c.x - in.inv_pose_xyz[0], c.y - in.inv_pose_xyz[1], c.z - in.inv_pose_xyz[2]));
        p.point[i3] = o.x; p.point[i3 + 1] = o.y; p.point[i3 + 2] = o.z;
    }
    if (p.normal) {
        const V3 n = pq_normal(p, in, best_slot);
        p.normal[i3] = n.x; p.normal[i3 + 1] = n.y; p.normal[i3 + 2] = n.z;
    }
    if (p.uv) {                                                 // w = (1 - b2) - b1, uv = (w uv0 + b1 uv1) + b2 uv2 (closest_point_kernel's)
        const float* t = p.tri_uv + (size_t)best_slot * 6;
        const float u0 = (1.0f - b2) - b1;
        p.uv[(size_t)i * 2] = (u0 * t[0] + b1 * t[2]) + b2 * t[4];
        p.uv[(size_t)i * 2 + 1] = (u0 * t[1] + b1 * t[3]) + b2 * t[5];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Triangle distance queries (rt_closest_to_triangles): the nearest point of the scene's triangles to each of the caller's triangles,
// equal bit for bit to a brute-force minimum over every (instance, triangle) -- rule 14 of include/rt_hip.h, the pruning argument in
// DESIGN.md section 19.  segment_closest_kernel's shape: one wave per workgroup, one query triangle per lane, the nearest-first
// traversal, the lower bound between the query's widened box and the child's.  The leaf is heavy (fifteen candidates: six
// pq_weights, nine sq_segseg), so all of it is one out-of-line routine that maps the query's vertices itself: the node loop holds
// the query's box and nothing else of the query.  The intersection half (step 5) is triangle_intersect_patch_kernel, after ti_trace.
// ---------------------------------------------------------------------------------------------------------
struct TdParams {
    const float4* records;
    const float* tri_uv;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* tris;          // [n][3][3] world query triangles
    const float* max_distance;  // [n] or null (= +inf)
    const int32_t* skip;        // [n] or null: one instance per query that contributes nothing (-1 = none)
    int32_t n;
    float* distance;            // outputs, each optional (null = not wanted)
    int32_t *instance, *triangle;
    float *query_barycentric, *query_point, *point, *normal, *barycentric, *uv;
    float* clearance;           // the distance here, set to 0 by triangle_intersect_patch_kernel where the triangle intersects
    int32_t* within;            // 1 where there is a candidate here, set to 1 by triangle_intersect_patch_kernel where it intersects
    int32_t* pops;
};

// query vertex k of triangle P (world, [3][3]) in instance in's scaled mesh space: apply_lre(pose, P_k), rule 1's map
__device__ __forceinline__ V3 td_vertex(const float* P, const DevInstance& in, int k)
{
    return apply_quat(in.q_pose, v3(P[3 * k] - in.pose_xyz[0], P[3 * k + 1] - in.pose_xyz[1], P[3 * k + 2] - in.pose_xyz[2]));
}

// One candidate (q1, q2, b1, b2) of a pair against the pair's best so far: the smaller d2, the earlier of equals; a NaN d2 never
// replaces one that is not NaN
struct TdCand { float q1, q2, b1, b2, d2; };
__device__ __forceinline__ void td_candidate(TdCand& best, V3 q0, V3 qab, V3 qac, V3 a, V3 ab, V3 ac, float q1, float q2, float b1,
                                             float b2)
{
    const float d2 = pq_d2(pq_combine(q0, qab, qac, q1, q2) - pq_combine(a, ab, ac, b1, b2));
    if (d2 < best.d2 || best.d2 != best.d2) { best.q1 = q1; best.q2 = q2; best.b1 = b1; best.b2 = b2; best.d2 = d2; }
}

// rule 14 steps 1-3 on one scene triangle: the query's vertices mapped again (the same sequence as the traversal's box), then the
// fifteen candidates in order.  Out of line and not unrolled -- one pq_weights and one call of sq_segseg in the code, whichever
// triangle is projected onto and whichever edges meet -- so none of it occupies the traversal's registers.
__device__ __noinline__ TdCand td_triangle(const float* P, const DevInstance& in, V3 a, V3 ab, V3 ac)
{
    const V3 q0 = td_vertex(P, in, 0);
    const V3 qab = td_vertex(P, in, 1) - q0, qac = td_vertex(P, in, 2) - q0;
    TdCand best;
    best.q1 = 0.0f; best.q2 = 0.0f; best.b1 = 0.0f; best.b2 = 0.0f; best.d2 = __int_as_float(0x7fc00000);
    // (a) 0-2: the query's vertices onto the scene triangle; (b) 3-5: the scene's vertices onto the query triangle, unless the query
    // is a point (then (a) alone: closest_point_kernel's answer)
    const bool spread = dot(qab, qab) > 0.0f || dot(qac, qac) > 0.0f;
#pragma unroll 1
    for (int k = 0; k < (spread ? 6 : 3); k++) {
        const bool onto_query = k >= 3;
        const int j = onto_query ? k - 3 : k;
        const V3 f0 = onto_query ? a : q0, f1 = onto_query ? ab : qab, f2 = onto_query ? ac : qac;       // the vertex comes from here
        const V3 t0 = onto_query ? q0 : a, t1 = onto_query ? qab : ab, t2 = onto_query ? qac : ac;       // and is projected onto this
        const V3 v = j == 0 ? f0 : (j == 1 ? f0 + f1 : f0 + f2);
        const float2 w = pq_weights(v, t0, t1, t2);
        const float u1 = j == 1 ? 1.0f : 0.0f, u2 = j == 2 ? 1.0f : 0.0f;
        if (onto_query) td_candidate(best, q0, qab, qac, a, ab, ac, w.x, w.y, u1, u2);
        else td_candidate(best, q0, qab, qac, a, ab, ac, u1, u2, w.x, w.y);
    }
    // (c) 6-14: query edge m against scene edge k, rule 13's closest pair
#pragma unroll 1
    for (int m = 0; m < 3; m++) {
        const V3 g0 = m == 2 ? q0 + qab : q0, d = m == 0 ? qab : (m == 1 ? qac : qac - qab);
        if (!(dot(d, d) > 0.0f)) continue;
#pragma unroll 1
        for (int k = 0; k < 3; k++) {
            const V3 e0 = k == 2 ? a + ab : a, f = k == 0 ? ab : (k == 1 ? ac : ac - ab);
            const float2 su = sq_segseg(g0, d, e0, f);
            const float s = su.x, u = su.y;
            td_candidate(best, q0, qab, qac, a, ab, ac, m == 0 ? s : (m == 1 ? 0.0f : 1.0f - s), m == 0 ? 0.0f : s,
                         k == 0 ? u : (k == 1 ? 0.0f : 1.0f - u), k == 0 ? 0.0f : u);
        }
    }
    return best;
}

// the query's interval on one axis over its three mapped vertices, widened by 2^-16 of their largest magnitude plus FLT_MIN: every
// computed X of rule 14 lies in it
__device__ __forceinline__ void td_interval(float a, float b, float c, float& lo, float& hi)
{
    const float m = fmaxf(fmaxf(fabsf(a), fabsf(b)), fabsf(c)) * 0x1p-16f + 0x1p-126f;
    lo = fminf(fminf(a, b), c) - m; hi = fmaxf(fmaxf(a, b), c) + m;
}

// ANY: only within and / or pops are wanted of this half: the traversal ends at the first candidate, across instances too
template <bool ANY>
__global__ __launch_bounds__(kPointBlock, 8) void triangle_closest_kernel(const TdParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kPointBlock]
    const int32_t i = (int32_t)blockIdx.x * kPointBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const size_t i3 = (size_t)i * 3;
    const float* P = p.tris + (size_t)i * 9;
    const float cut2 = pq_cut2(p.max_distance ? p.max_distance[i] : __int_as_float(0x7f800000));
    const int32_t skip = p.skip ? p.skip[i] : -1;
    int spill[kMaxStack - kLdsStack];
    PointStack stack = query_stack(lds_stack, spill, p.stack_depth);
    // the best candidate so far by (d2, instance, tri_id); best_inst < 0 = none yet
    float best = 0.0f, bq1 = 0.0f, bq2 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    int32_t best_inst = -1, best_slot = 0, best_tid = 0, pops = 0;
    for (int32_t k = 0; k < p.num_instances && cut2 >= 0.0f && !(ANY && best_inst >= 0); k++) {
        if (k == skip) continue;
        const DevInstance& in = p.instances[k];
        V3 slo, shi;
        {                                                       // (the mapped vertices live only here: the leaf maps them again)
            const V3 q0 = td_vertex(P, in, 0), q1 = td_vertex(P, in, 1), q2 = td_vertex(P, in, 2);
            td_interval(q0.x, q1.x, q2.x, slo.x, shi.x); td_interval(q0.y, q1.y, q2.y, slo.y, shi.y);
            td_interval(q0.z, q1.z, q2.z, slo.z, shi.z);
        }
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: both child boxes, nearer first
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const float la = sq_box_lb(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, slo, shi);
                const float lb = sq_box_lb(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, slo, shi);
                const float lim = best_inst >= 0 ? best : cut2;
                const bool pa = !(prune && la > lim), pb = !(prune && lb > lim);
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                const bool a_near = !(lb < la);
                if (pa && pb) stack.push(a_near ? rb : ra);
                cur = (pa && pb) ? (a_near ? ra : rb) : (pa ? ra : (pb ? rb : kNeedPop));
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    const float4 t0 = rec[0], t1 = rec[1], t2 = rec[2];
                    V3 a, ab, ac;
                    pq_triangle(t0, t1, t2, s, a, ab, ac);
                    const TdCand c = td_triangle(P, in, a, ab, ac);
                    if (c.d2 <= (best_inst >= 0 ? best : cut2)) {   // (NaN fails)
                        const int32_t tid = p.tri_id[slot];
                        if (best_inst < 0 || c.d2 < best || (best_inst == k && tid < best_tid)) {
                            best = c.d2; bq1 = c.q1; bq2 = c.q2; b1 = c.b1; b2 = c.b2; best_inst = k; best_slot = slot; best_tid = tid;
                        }
                    }
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel && !(ANY && best_inst >= 0));
    }
    const bool got = best_inst >= 0;
    if (p.pops) p.pops[i] = pops;
    if (p.within) p.within[i] = got ? 1 : 0;
    if constexpr (ANY) return;
    const float dist = got ? sqrtf(best) : FLT_MAX;
    if (p.distance) p.distance[i] = dist;
    if (p.clearance) p.clearance[i] = dist;
    if (p.instance) p.instance[i] = got ? best_inst : -1;
    if (p.triangle) p.triangle[i] = got ? best_tid : -1;
    if (p.query_barycentric) { p.query_barycentric[(size_t)i * 2] = got ? bq1 : 0.0f; p.query_barycentric[(size_t)i * 2 + 1] = got ? bq2 : 0.0f; }
    if (p.barycentric) { p.barycentric[(size_t)i * 2] = got ? b1 : 0.0f; p.barycentric[(size_t)i * 2 + 1] = got ? b2 : 0.0f; }
    if (!got) {
        if (p.query_point) { p.query_point[i3] = 0.0f; p.query_point[i3 + 1] = 0.0f; p.query_point[i3 + 2] = 0.0f; }
        if (p.point) { p.point[i3] = 0.0f; p.point[i3 + 1] = 0.0f; p.point[i3 + 2] = 0.0f; }
        if (p.normal) { p.normal[i3] = 0.0f; p.normal[i3 + 1] = 0.0f; p.normal[i3 + 2] = 0.0f; }
        if (p.uv) { p.uv[(size_t)i * 2] = 0.0f; p.uv[(size_t)i * 2 + 1] = 0.0f; }
        return;
    }
    const DevInstance& in = p.instances[best_inst];
    if (p.query_point) {                                        // the winner's X again (same sequence), to world: apply_lre(inv_pose, X)
        const V3 q0 = td_vertex(P, in, 0);
        const V3 x = pq_combine(q0, td_vertex(P, in, 1) - q0, td_vertex(P, in, 2) - q0, bq1, bq2);
        const V3 o = apply_quat(in.q_inv_pose, v3(x.x - in.inv_pose_xyz[0], x.y - in.inv_pose_xyz[1], x.z - in.inv_pose_xyz[2]));
        p.query_point[i3] = o.x; p.query_point[i3 + 1] = o.y; p.query_point[i3 + 2] = o.z;
    }
    if (p.point) {                                              // the winner's c again (same sequence), closest_point_kernel's map
        const float4* rec = p.records + (size_t)best_slot * 4;
        V3 a, ab, ac;
        pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
        const V3 c = pq_combine(a, ab, ac, b1, b2);
        const V3 o = apply_quat(in.q_inv_pose, v3(c.x - in.inv_pose_xyz[0], c.y - in.inv_pose_xyz[1], c.z - in.inv_pose_xyz[2]));
        p.point[i3] = o.x; p.point[i3 + 1] = o.y; p.point[i3 + 2] = o.z;
    }
    if (p.normal) {
        const V3 n = pq_normal(p, in, best_slot);
        p.normal[i3] = n.x; p.normal[i3 + 1] = n.y; p.normal[i3 + 2] = n.z;
    }
    if (p.uv) {                                                 // w = (1 - b2) - b1, uv = (w uv0 + b1 uv1) + b2 uv2 (closest_point_kernel's)
        const float* t = p.tri_uv + (size_t)best_slot * 6;
        const float u0 = (1.0f - b2) - b1;
        p.uv[(size_t)i * 2] = (u0 * t[0] + b1 * t[2]) + b2 * t[4];
        p.uv[(size_t)i * 2 + 1] = (u0 * t[1] + b1 * t[3]) + b2 * t[5];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Sphere sweeps (rt_sweep_spheres): the first contact of a sphere of radius r whose centre moves from P0 to P1, equal bit for bit to
// a brute-force loop over every (instance, triangle) -- rule 16 of include/rt_hip.h, the pruning argument in DESIGN.md section 22.
// segment_closest_kernel's shape: one wave per workgroup, one sweep per lane, the general stack, instances in ascending order.  The
// lower bound is between the child's box and the box of the path up to the best time so far, which shrinks as the winner improves;
// the children are visited nearer-to-Q0 first.  The leaf (eight candidate times, each priced by pq_weights) is one out-of-line
// routine that maps the ends itself, as td_triangle does: the node loop holds the path's box, Q0 and the bound, nothing else.
// ---------------------------------------------------------------------------------------------------------
struct SweepParams {
    const float4* records;
    const float* tri_uv;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* segs;          // [n][2][3] world positions of the centre: P0 then P1
    const float* radius;        // [n]
    int32_t n;
    float *time, *distance;     // outputs, each optional (null = not wanted)
    int32_t *instance, *triangle;
    float *centre, *point, *normal, *contact_normal, *barycentric, *uv;
    int32_t *hit, *pops;
};

// rule 16 step 3's constants: reach = (r + r * kSweepKR) + M * kSweepKM (DESIGN.md section 22 has the measurement that fixes them)
constexpr float kSweepKR = 0x1p-20f, kSweepKM = 0x1p-20f;

__device__ __forceinline__ float sw_absmax(float m, float x) { const float a = fabsf(x); return a > m ? a : m; }      // (a NaN is passed over)
__device__ __forceinline__ float sw_reach2(float r, V3 q0, V3 q1)
{
    float m = 0.0f;
    m = sw_absmax(m, q0.x); m = sw_absmax(m, q0.y); m = sw_absmax(m, q0.z);
    m = sw_absmax(m, q1.x); m = sw_absmax(m, q1.y); m = sw_absmax(m, q1.z);
    const float rw = (r + r * kSweepKR) + m * kSweepKM;
    return rw * rw;
}
// the ends g = (P0, P1) in instance `in`'s scaled mesh space (read again wherever they are needed: not held across the traversal)
__device__ __forceinline__ void sw_ends(const float* g, const DevInstance& in, V3& q0, V3& q1)
{
    q0 = apply_quat(in.q_pose, v3(g[0] - in.pose_xyz[0], g[1] - in.pose_xyz[1], g[2] - in.pose_xyz[2]));
    q1 = apply_quat(in.q_pose, v3(g[3] - in.pose_xyz[0], g[4] - in.pose_xyz[1], g[5] - in.pose_xyz[2]));
}
__device__ __forceinline__ V3 sw_along(V3 p, float s, V3 d) { return v3(p.x + s * d.x, p.y + s * d.y, p.z + s * d.z); }
__device__ __forceinline__ V3 sw_off(V3 p, float s, V3 d) { return v3(p.x - s * d.x, p.y - s * d.y, p.z - s * d.z); }

// rule 16 steps 2-3 on one scene triangle: (s, b1, b2, d2) of its candidate, s = -1 when it has none.  lim: the lane's best time so
// far (1 without one); a candidate time above it cannot win and is not priced.  Out of line and not unrolled: one pq_weights in the
// code whichever candidate is priced.
__device__ __noinline__ float4 sw_triangle(const float* g, float r, const DevInstance& in, V3 a, V3 ab, V3 ac, float lim)
{
    V3 q0, q1;
    sw_ends(g, in, q0, q1);
    const float reach2 = sw_reach2(r, q0, q1), r2 = r * r;
    const V3 d = q1 - q0;
    const float aa = dot(d, d);
    float4 best = make_float4(-1.0f, 0.0f, 0.0f, 0.0f);
    const int count = aa > 0.0f ? 8 : 1;                        // (a zero-length sweep has the start alone)
#pragma unroll 1
    for (int k = 0; k < count; k++) {
        float s = __int_as_float(0x7fc00000);                   // (no root: fails the compares below)
        if (k == 0) {
            s = 0.0f;
        } else if (k == 1) {                                    // the face: the plane offset by r on Q0's side, approached
            const V3 n = v3(ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x);
            const float m = sw_absmax(sw_absmax(sw_absmax(0.0f, n.x), n.y), n.z);
            if (m > 0.0f) {
                const V3 u = v3(n.x / m, n.y / m, n.z / m);
                const float lu = sqrtf(pq_d2(u)), h0 = dot(u, q0 - a), vn = dot(u, d);
                float gap = 0.0f, v = 0.0f;
                if (h0 >= 0.0f) { gap = h0 - r * lu; v = -vn; }
                else if (h0 < 0.0f) { gap = -h0 - r * lu; v = vn; }
                if (v > 0.0f) s = gap / v;
            }
        } else if (k < 5) {                                     // an edge's line: the cylinder of radius r about it, entry root
            const V3 e0 = k == 4 ? a + ab : a, f = k == 2 ? ab : (k == 3 ? ac : ac - ab);
            const float ff = dot(f, f);
            if (ff > 0.0f) {
                const V3 w = q0 - e0;
                const float td = dot(d, f) / ff, tw = dot(w, f) / ff;
                const V3 dp = sw_off(d, td, f), wp = sw_off(w, tw, f);
                const float ap = dot(dp, dp);
                if (ap > 0.0f) {
                    const float smid = -dot(wp, dp) / ap, dp2 = pq_d2(sw_along(wp, smid, dp));
                    if (dp2 <= r2) s = smid - sqrtf((r2 - dp2) / ap);
                }
            }
        } else {                                                // a vertex: the sphere of radius r about it, entry root
            const V3 w = q0 - (k == 5 ? a : (k == 6 ? a + ab : a + ac));
            const float smid = -dot(w, d) / aa, dp2 = pq_d2(sw_along(w, smid, d));
            if (dp2 <= r2) s = smid - sqrtf((r2 - dp2) / aa);
        }
        if (!(s >= 0.0f && s <= lim)) continue;                 // (lim <= 1; a NaN fails)
        if (best.x >= 0.0f && !(s < best.x)) continue;          // (the first of equals stays)
        const V3 x = sw_along(q0, s, d);
        const float2 bw = pq_weights(x, a, ab, ac);
        const float d2 = pq_d2(x - pq_combine(a, ab, ac, bw.x, bw.y));
        if (d2 <= reach2) {                                     // step 3: valid (a NaN fails)
            best = make_float4(s, bw.x, bw.y, d2);
            if (k == 0) break;                                  // (nothing is earlier than the start)
        }
    }
    return best;
}

// the box of the path from Q0 to the end of what can still win -- Q1 without a winner, else E = Q0 + s_lim * D as rule 16 computes an
// X (every X with s <= s_lim lies between Q0 and E per axis: rounding is monotone) -- widened as sq_interval does it; Q0; step 3's bound
__device__ __forceinline__ void sw_path(const float* g, const DevInstance& in, float r, bool got, float s_lim, V3& slo, V3& shi, V3& q0,
                                        float& reach2)
{
    V3 q1;
    sw_ends(g, in, q0, q1);
    reach2 = sw_reach2(r, q0, q1);
    if (got) q1 = sw_along(q0, s_lim, q1 - q0);
    sq_interval(q0.x, q1.x, slo.x, shi.x); sq_interval(q0.y, q1.y, slo.y, shi.y); sq_interval(q0.z, q1.z, slo.z, shi.z);
}

// ANY: only hit and / or pops are wanted: the traversal ends at the first valid candidate, across instances too
template <bool ANY>
__global__ __launch_bounds__(kPointBlock, 8) void sweep_kernel(const SweepParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kPointBlock]
    const int32_t i = (int32_t)blockIdx.x * kPointBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const size_t i3 = (size_t)i * 3;
    const float* g = p.segs + (size_t)i * 6;
    const float r = p.radius[i];
    int spill[kMaxStack - kLdsStack];
    PointStack stack = query_stack(lds_stack, spill, p.stack_depth);
    // the best candidate so far by (s, d2, instance, tri_id); best_inst < 0 = none yet
    float bs = 1.0f, best = 0.0f, b1 = 0.0f, b2 = 0.0f;
    int32_t best_inst = -1, best_slot = 0, best_tid = 0, pops = 0;
    for (int32_t k = 0; k < p.num_instances && r >= 0.0f && !(ANY && best_inst >= 0); k++) {       // (a NaN or negative radius: no contact)
        const DevInstance& in = p.instances[k];
        V3 slo, shi, q0;
        float reach2;
        sw_path(g, in, r, best_inst >= 0, bs, slo, shi, q0, reach2);
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: both child boxes, nearer to Q0 first
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const float la = sq_box_lb(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, slo, shi);
                const float lb = sq_box_lb(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, slo, shi);
                // a contact at time 0 is beaten only by a smaller d2 at time 0 (equal is kept); otherwise by anything valid in the box
                const float lim = (best_inst >= 0 && bs == 0.0f) ? best : reach2;
                const bool pa = !(prune && la > lim), pb = !(prune && lb > lim);
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                bool a_near = true;
                if (pa && pb) {
                    a_near = !(pq_box_lb(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, q0) < pq_box_lb(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, q0));
                    stack.push(a_near ? rb : ra);
                }
                cur = (pa && pb) ? (a_near ? ra : rb) : (pa ? ra : (pb ? rb : kNeedPop));
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    const float4 t0 = rec[0], t1 = rec[1], t2 = rec[2];
                    V3 a, ab, ac;
                    pq_triangle(t0, t1, t2, s, a, ab, ac);
                    const float4 c = sw_triangle(g, r, in, a, ab, ac, bs);
                    if (c.x >= 0.0f) {                          // a valid candidate at a time <= bs
                        const int32_t tid = p.tri_id[slot];
                        const bool sooner = best_inst < 0 || c.x < bs;
                        if (sooner || c.w < best || (c.w == best && best_inst == k && tid < best_tid)) {
                            bs = c.x; best = c.w; b1 = c.y; b2 = c.z; best_inst = k; best_slot = slot; best_tid = tid;
                            if (sooner && !ANY) sw_path(g, in, r, true, bs, slo, shi, q0, reach2);  // the path's box shrinks
                        }
                    }
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel && !(ANY && best_inst >= 0));
    }
    const bool got = best_inst >= 0;
    if (p.pops) p.pops[i] = pops;
    if (p.hit) p.hit[i] = got ? 1 : 0;
    if constexpr (ANY) return;
    if (p.time) p.time[i] = got ? bs : FLT_MAX;
    if (p.distance) p.distance[i] = got ? sqrtf(best) : FLT_MAX;
    if (p.instance) p.instance[i] = got ? best_inst : -1;
    if (p.triangle) p.triangle[i] = got ? best_tid : -1;
    if (p.barycentric) { p.barycentric[(size_t)i * 2] = got ? b1 : 0.0f; p.barycentric[(size_t)i * 2 + 1] = got ? b2 : 0.0f; }
    if (!got) {
        if (p.centre) { p.centre[i3] = 0.0f; p.centre[i3 + 1] = 0.0f; p.centre[i3 + 2] = 0.0f; }
        if (p.point) { p.point[i3] = 0.0f; p.point[i3 + 1] = 0.0f; p.point[i3 + 2] = 0.0f; }
        if (p.normal) { p.normal[i3] = 0.0f; p.normal[i3 + 1] = 0.0f; p.normal[i3 + 2] = 0.0f; }
        if (p.contact_normal) { p.contact_normal[i3] = 0.0f; p.contact_normal[i3 + 1] = 0.0f; p.contact_normal[i3 + 2] = 0.0f; }
        if (p.uv) { p.uv[(size_t)i * 2] = 0.0f; p.uv[(size_t)i * 2 + 1] = 0.0f; }
        return;
    }
    const DevInstance& in = p.instances[best_inst];
    V3 fn = v3(0.0f, 0.0f, 0.0f);
    if (p.normal || p.contact_normal) fn = pq_normal(p, in, best_slot);
    if (p.normal) { p.normal[i3] = fn.x; p.normal[i3 + 1] = fn.y; p.normal[i3 + 2] = fn.z; }
    if (p.centre || p.point || p.contact_normal) {              // the winner's X and c again (the same sequences)
        V3 q0, q1, a, ab, ac;
        sw_ends(g, in, q0, q1);
        const V3 x = sw_along(q0, bs, q1 - q0);
        const float4* rec = p.records + (size_t)best_slot * 4;
        pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
        const V3 c = pq_combine(a, ab, ac, b1, b2);
        if (p.centre) {                                         // to world: apply_lre(inv_pose, X), segment_point's map
            const V3 o = apply_quat(in.q_inv_pose, v3(x.x - in.inv_pose_xyz[0], x.y - in.inv_pose_xyz[1], x.z - in.inv_pose_xyz[2]));
            p.centre[i3] = o.x; p.centre[i3 + 1] = o.y; p.centre[i3 + 2] = o.z;
        }
        if (p.point) {
            const V3 o = apply_quat(in.q_inv_pose, v3(c.x - in.inv_pose_xyz[0], c.y - in.inv_pose_xyz[1], c.z - in.inv_pose_xyz[2]));
            p.point[i3] = o.x; p.point[i3 + 1] = o.y; p.point[i3 + 2] = o.z;
        }
        if (p.contact_normal) {                                 // (X - c) / sqrtf(d2) rotated to world; the face normal where d2 is not > 0
            if (best > 0.0f) {
                const float len = sqrtf(best);
                const V3 e = x - c;
                fn = apply_quat(in.q_inv_rot, v3(e.x / len, e.y / len, e.z / len));
            }
            p.contact_normal[i3] = fn.x; p.contact_normal[i3 + 1] = fn.y; p.contact_normal[i3 + 2] = fn.z;
        }
    }
    if (p.uv) {                                                 // w = (1 - b2) - b1, uv = (w uv0 + b1 uv1) + b2 uv2 (closest_point_kernel's)
        const float* t = p.tri_uv + (size_t)best_slot * 6;
        const float u0 = (1.0f - b2) - b1;
        p.uv[(size_t)i * 2] = (u0 * t[0] + b1 * t[2]) + b2 * t[4];
        p.uv[(size_t)i * 2 + 1] = (u0 * t[1] + b1 * t[3]) + b2 * t[5];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Ray crossing counts and winding numbers (rt_count_crossings / rt_winding_numbers / rt_signed_distance): every triangle a ray
// crosses within (0, tmax], both faces, with the sign of the crossing -- equal to a brute-force count over every (instance,
// triangle); the rule is in include/rt_hip.h, the pruning argument in DESIGN.md section 12.  One wave per workgroup, one ray (or
// point) per lane, an unordered traversal of each instance's tree on the general stack: every child the ray may cross is visited.
// ---------------------------------------------------------------------------------------------------------
struct CrossParams {
    const float4* records;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* org;           // [n][3] ray origins (the point form: the points)
    const float* dir;           // [n][3] ray directions (the point form: unused)
    const float* tmax;          // [n] or null (= +inf; the point form: unused)
    int32_t n;
    int32_t *count, *winding, *pops;    // outputs, each optional (the point form: winding = the median winding; no count, no pops)
    float* sdf;                 // the point form: holds rt_closest_points' distance, negated where the winding is not 0
};
constexpr int kCrossBlock = 64;
typedef StackT<kCrossBlock> CrossStack;

__device__ __forceinline__ float xq_sel(V3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// The exact signs of U, V, W when the fp32 ones hold a zero: the products of fp32 values are exact in fp64, and a nonzero difference
// that rounds to 0 in fp32 (below 2^-150) becomes +-2^-149, so the sign survives the rounding (rare: out of line)
__device__ __forceinline__ float xq_narrow(double x)
{
    const float f = (float)x;
    return f == 0.0f && x != 0.0 ? (x > 0.0 ? 0x1p-149f : -0x1p-149f) : f;
}
__device__ __noinline__ float3 xq_edges64(float ax, float ay, float bx, float by, float cx, float cy)
{
    return make_float3(xq_narrow((double)cx * (double)by - (double)cy * (double)bx), xq_narrow((double)ax * (double)cy - (double)ay * (double)cx),
                       xq_narrow((double)bx * (double)ay - (double)by * (double)ax));
}

// The ray in one instance's scaled mesh space, set up for the watertight test (Woop, Benthin, Wald, JCGT 2(1) 2013)
struct XqRay {
    V3 o;                       // o' = apply_lre(pose, o)
    float ox, oy, oz;           // o' permuted to (kx, ky, kz)
    float sx, sy, sz;           // the shear constants
    V3 inv;                     // 1 / d' per axis (the slab test)
    int kx, ky, kz;
    float omax;                 // max_k |o'_k| (NaN-free: fmaxf)
    bool zero;                  // d' == 0
};

// rule 3's set-up from a mesh-space o' and d': the shear axes and constants (the slab terms inv and omax are left unset)
__device__ __forceinline__ void xq_shear(XqRay& r, V3 o, V3 dd)
{
    r.o = o;
    const float ax = fabsf(dd.x), ay = fabsf(dd.y), az = fabsf(dd.z);
    int kz = 0;
    float m = ax;
    if (ay > m) { kz = 1; m = ay; }
    if (az > m) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = xq_sel(dd, kz);
    r.zero = dz == 0.0f;
    if (dz < 0.0f) { const int t = kx; kx = ky; ky = t; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.sx = xq_sel(dd, kx) / dz; r.sy = xq_sel(dd, ky) / dz; r.sz = 1.0f / dz;
    r.ox = xq_sel(r.o, kx); r.oy = xq_sel(r.o, ky); r.oz = xq_sel(r.o, kz);
}

__device__ __forceinline__ XqRay xq_ray(const DevInstance& in, V3 w, V3 d)
{
    XqRay r;
    const V3 o = apply_quat(in.q_pose, v3(w.x - in.pose_xyz[0], w.y - in.pose_xyz[1], w.z - in.pose_xyz[2]));
    const V3 dd = apply_quat(in.q_pose, d);
    xq_shear(r, o, dd);
    r.inv = v3(1.0f / dd.x, 1.0f / dd.y, 1.0f / dd.z);
    r.omax = fmaxf(fmaxf(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z));
    return r;
}

// rule 3 of include/rt_hip.h on the triangle given by its vertices (a, b, c): 0 = not counted, else the sign of the crossing (+1
// leaving); on a counted triangle also t, V, W and det (b1 = V / det, b2 = W / det)
__device__ __forceinline__ int xq_vertices(const XqRay& r, V3 a, V3 b, V3 c, float tmax, float& t_out, float& v_out, float& w_out,
                                           float& det_out)
{
    const float az = xq_sel(a, r.kz) - r.oz, bz = xq_sel(b, r.kz) - r.oz, cz = xq_sel(c, r.kz) - r.oz;
    const float ax = (xq_sel(a, r.kx) - r.ox) - r.sx * az, ay = (xq_sel(a, r.ky) - r.oy) - r.sy * az;
    const float bx = (xq_sel(b, r.kx) - r.ox) - r.sx * bz, by = (xq_sel(b, r.ky) - r.oy) - r.sy * bz;
    const float cx = (xq_sel(c, r.kx) - r.ox) - r.sx * cz, cy = (xq_sel(c, r.ky) - r.oy) - r.sy * cz;
    float u = cx * by - cy * bx, v = ax * cy - ay * cx, w = bx * ay - by * ax;
    if (u == 0.0f || v == 0.0f || w == 0.0f) {
        const float3 e = xq_edges64(ax, ay, bx, by, cx, cy);
        u = e.x; v = e.y; w = e.z;
    }
    const bool neg = u <= 0.0f && v <= 0.0f && w <= 0.0f, pos = u >= 0.0f && v >= 0.0f && w >= 0.0f;
    const float det = (u + v) + w;
    if (!(neg || pos) || det == 0.0f) return 0;
    const float T = (u * (r.sz * az) + v * (r.sz * bz)) + w * (r.sz * cz);
    const float t = T / det;
    if (!(t > 0.0f && t <= tmax)) return 0;
    t_out = t; v_out = v; w_out = w; det_out = det;
    return det < 0.0f ? 1 : -1;
}

// rule 3 on the triangle (A, A + AB, A + AC): 0 = not counted, else the sign of the crossing (+1 leaving)
__device__ __forceinline__ int xq_triangle(const XqRay& r, V3 a, V3 ab, V3 ac, float tmax)
{
    float t, v, w, det;
    return xq_vertices(r, a, a + ab, a + ac, tmax, t, v, w, det);
}

// Whether a counted triangle may lie in the mesh-space box lo..hi: the box is scaled (a negative scale swaps
// the ends) and widened by 2^-16 of (its largest coordinate magnitude + the origin's) plus FLT_MIN; it is kept when the ray's line
// meets it (an axis whose slab gives a NaN does not constrain) and its kz slab is not wholly behind the origin.  Boxes with a
// coordinate magnitude above 2^60 (or a NaN one) are always kept.
__device__ __forceinline__ bool xq_box(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, const XqRay& r)
{
    const float x0 = lx * s.x, x1 = hx * s.x, y0 = ly * s.y, y1 = hy * s.y, z0 = lz * s.z, z1 = hz * s.z;
    const float bmax = fmaxf(fmaxf(fmaxf(fabsf(x0), fabsf(x1)), fmaxf(fabsf(y0), fabsf(y1))), fmaxf(fabsf(z0), fabsf(z1)));
    if (!(bmax <= 0x1p60f)) return true;
    const float m = (bmax + r.omax) * 0x1p-16f + 0x1p-126f;
    float tn = -__int_as_float(0x7f800000), tf = __int_as_float(0x7f800000), fz = tf;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float a = k == 0 ? x0 : (k == 1 ? y0 : z0), b = k == 0 ? x1 : (k == 1 ? y1 : z1);
        const float o = k == 0 ? r.o.x : (k == 1 ? r.o.y : r.o.z), inv = k == 0 ? r.inv.x : (k == 1 ? r.inv.y : r.inv.z);
        const float t1 = ((fminf(a, b) - m) - o) * inv, t2 = ((fmaxf(a, b) + m) - o) * inv;
        if (t1 == t1 && t2 == t2) {                             // (a NaN slab: no constraint)
            tn = fmaxf(tn, fminf(t1, t2));
            const float f = fmaxf(t1, t2);
            tf = fminf(tf, f);
            if (k == r.kz) fz = f;
        }
    }
    return !(tn > tf) && !(fz < 0.0f);
}

// One ray through every instance: count, winding and pops of rule 5; P: CrossParams or SegParams
template <typename P>
__device__ __forceinline__ void xq_trace(const P& p, CrossStack& stack, V3 w, V3 d, float tmax, int32_t& count,
                                         int32_t& winding, int32_t& pops)
{
    for (int32_t k = 0; k < p.num_instances; k++) {
        const DevInstance& in = p.instances[k];
        const XqRay r = xq_ray(in, w, d);
        if (r.zero) continue;                                   // (a zero d' counts nothing)
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        // (an origin beyond 2^60: no pruning in this instance either); the child boxes the ray may cross
        walk_unordered(p, stack, in, boxes_ordered(p, in) && r.omax <= 0x1p60f, pops,
                       [&](float lx, float ly, float lz, float hx, float hy, float hz) {
            return xq_box(lx, ly, lz, hx, hy, hz, s, r);
        }, [&](int32_t, float4 t0, float4 t1, float4 t2) {
            V3 a, ab, ac;
            pq_triangle(t0, t1, t2, s, a, ab, ac);
            const int sign = xq_triangle(r, a, ab, ac, tmax);
            count += sign != 0 ? 1 : 0;
            winding += sign;
            return false;
        });
    }
}

// POINT = false: rt_count_crossings, one ray per lane.  POINT = true: rt_winding_numbers / rt_signed_distance, one point per lane,
// the median of the windings along RT_WINDING_D1..D3 (one kernel, two instantiations: the point form only adds the loop over the
// three directions around the same traversal).
template <bool POINT>
__global__ __launch_bounds__(kCrossBlock, 8) void crossing_kernel(const CrossParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kCrossBlock]
    const int32_t i = (int32_t)blockIdx.x * kCrossBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const size_t i3 = (size_t)i * 3;
    const V3 w = v3(p.org[i3], p.org[i3 + 1], p.org[i3 + 2]);
    int spill[kMaxStack - kLdsStack];
    CrossStack stack = query_stack(lds_stack, spill, p.stack_depth);
    int32_t count = 0, winding = 0, pops = 0;
    if constexpr (!POINT) {
        const float tmax = p.tmax ? p.tmax[i] : __int_as_float(0x7f800000);
        xq_trace(p, stack, w, v3(p.dir[i3], p.dir[i3 + 1], p.dir[i3 + 2]), tmax, count, winding, pops);
        if (p.count) p.count[i] = count;
        if (p.winding) p.winding[i] = winding;
        if (p.pops) p.pops[i] = pops;
    } else {
        constexpr float d1[3] = RT_WINDING_D1, d2[3] = RT_WINDING_D2, d3[3] = RT_WINDING_D3;
        int32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            const V3 d = j == 0 ? v3(d1[0], d1[1], d1[2]) : (j == 1 ? v3(d2[0], d2[1], d2[2]) : v3(d3[0], d3[1], d3[2]));
            int32_t c = 0, wj = 0;
            xq_trace(p, stack, w, d, __int_as_float(0x7f800000), c, wj, pops);
            w0 = j == 0 ? wj : w0; w1 = j == 1 ? wj : w1; w2 = j == 2 ? wj : w2;
        }
        const int32_t med = max(min(w0, w1), min(max(w0, w1), w2));
        if (p.winding) p.winding[i] = med;
        if (p.sdf && med != 0) p.sdf[i] = -p.sdf[i];
    }
}

// The crossing half of rt_closest_to_segments (rule 13 step 6): rt_count_crossings' count for the ray o = P0, d = P1 - P0, tmax = 1, one
// segment per lane, patching what segment_closest_kernel wrote on the same stream -- clearance becomes 0 and within 1 where the
// segment crosses a triangle (as the point form above patches sdf).  A lane whose answer cannot change any more does not traverse.
__global__ __launch_bounds__(kCrossBlock, 8) void segment_crossing_kernel(const SegParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kCrossBlock]
    const int32_t i = (int32_t)blockIdx.x * kCrossBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    if (!p.crossings && !p.clearance && p.within[i] != 0) return;   // (within alone, and the distance half has already said 1)
    const float* g = p.segs + (size_t)i * 6;
    const V3 w = v3(g[0], g[1], g[2]);
    int spill[kMaxStack - kLdsStack];
    CrossStack stack = query_stack(lds_stack, spill, p.stack_depth);
    int32_t count = 0, winding = 0, pops = 0;
    xq_trace(p, stack, w, v3(g[3] - w.x, g[4] - w.y, g[5] - w.z), 1.0f, count, winding, pops);
    if (p.crossings) p.crossings[i] = count;
    if (count > 0) {
        if (p.clearance) p.clearance[i] = 0.0f;
        if (p.within) p.within[i] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Crossing lists (rt_crossing_offsets / rt_list_crossings): every counted (instance, triangle) pair of rt_count_crossings, in the
// order (t, instance, triangle), written into the ray's own room of the output (include/rt_hip.h rule 8).
// The traversal is xq_trace's (same XqRay, xq_box and pruning), so the set of pairs is count_crossings' set.
// ---------------------------------------------------------------------------------------------------------
struct CrossListParams {
    const float4* records;
    const float* tri_uv;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* org;           // [n][3] ray origins
    const float* dir;           // [n][3] ray directions
    const float* tmax;          // [n] or null (= +inf)
    int32_t n;
    const int64_t* offsets;     // [n + 1] (CSR rooms) or null: fixed rooms of max_hits
    int32_t max_hits;
    float* t;                   // outputs, each optional (indexed by room slot; count by ray)
    int32_t *instance, *triangle;
    int8_t* sign;
    float *barycentric, *uv, *point;
    int32_t* count;
};

// xq_triangle with what the list needs of the test: on a counted triangle also t, V, W and det (b1 = V / det, b2 = W / det)
__device__ __forceinline__ int xq_triangle_uvw(const XqRay& r, V3 a, V3 ab, V3 ac, float tmax, float& t_out, float& v_out, float& w_out,
                                               float& det_out)
{
    return xq_vertices(r, a, a + ab, a + ac, tmax, t_out, v_out, w_out, det_out);
}

// xq_trace's traversal, calling hit(k, slot, t, v, w, det, sign) at each counted triangle (instances in ascending order, triangles of
// one instance in tree order).  The ray is read again at each instance, so it is not held in registers across the traversal.
template <typename Hit>
__device__ __forceinline__ void xl_trace(const CrossListParams& p, CrossStack& stack, size_t i3, float tmax, Hit&& hit)
{
    for (int32_t k = 0; k < p.num_instances; k++) {
        const DevInstance& in = p.instances[k];
        const XqRay r = xq_ray(in, v3(p.org[i3], p.org[i3 + 1], p.org[i3 + 2]), v3(p.dir[i3], p.dir[i3 + 1], p.dir[i3 + 2]));
        if (r.zero) continue;
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        int32_t pops = 0;                                       // (not reported)
        walk_unordered(p, stack, in, boxes_ordered(p, in) && r.omax <= 0x1p60f, pops,
                       [&](float lx, float ly, float lz, float hx, float hy, float hz) {
            return xq_box(lx, ly, lz, hx, hy, hz, s, r);
        }, [&](int32_t slot, float4 t0, float4 t1, float4 t2) {
            V3 a, ab, ac;
            pq_triangle(t0, t1, t2, s, a, ab, ac);
            float t = 0.0f, tv = 0.0f, tw = 0.0f, det = 1.0f;
            const int sign = xq_triangle_uvw(r, a, ab, ac, tmax, t, tv, tw, det);
            if (sign != 0) hit(k, slot, t, tv, tw, det, sign);
            return false;
        });
    }
}

// ray i's room: start and size (CSR: offsets[i] and offsets[i+1] - offsets[i], 0 when not positive; fixed: i*K and K); P:
// CrossListParams or NearbyParams
template <typename P>
__device__ __forceinline__ void xl_room(const P& p, int32_t i, size_t& start, uint64_t& room)
{
    if (p.offsets) {
        const int64_t s0 = p.offsets[i], s1 = p.offsets[i + 1];
        start = (size_t)s0;
        room = s1 > s0 ? (uint64_t)s1 - (uint64_t)s0 : 0u;
    } else {
        start = (size_t)i * (size_t)p.max_hits;
        room = (uint64_t)p.max_hits;
    }
}

// one entry of a room: slot j (absolute) <- the counted pair (k, slot) of ray i
__device__ __forceinline__ void xl_store(const CrossListParams& p, size_t j, int32_t i, int32_t k, int32_t slot, int32_t tid, float t, float b1,
                                         float b2, int sign)
{
    if (p.t) p.t[j] = t;
    if (p.instance) p.instance[j] = k;
    if (p.triangle) p.triangle[j] = tid;
    if (p.sign) p.sign[j] = (int8_t)sign;
    if (p.barycentric) { p.barycentric[2 * j] = b1; p.barycentric[2 * j + 1] = b2; }
    if (p.uv) {                                                 // w = (1 - b2) - b1, uv = (w uv0 + b1 uv1) + b2 uv2 (rt_closest_points')
        const float* q = p.tri_uv + (size_t)slot * 6;
        const float u0 = (1.0f - b2) - b1;
        p.uv[2 * j] = (u0 * q[0] + b1 * q[2]) + b2 * q[4];
        p.uv[2 * j + 1] = (u0 * q[1] + b1 * q[3]) + b2 * q[5];
    }
    if (p.point) {                                              // o + t*d per component, world
        const size_t i3 = (size_t)i * 3;
        for (int c = 0; c < 3; c++) p.point[3 * j + c] = p.org[i3 + c] + t * p.dir[i3 + c];
    }
}

// SELECT = false (t, instance and triangle all given): one traversal, each counted pair inserted into the room, which stays sorted
// by (t, instance, triangle) -- lane-private, no atomics; once the room is full a pair enters only below the last entry.
// SELECT = true (a key field not given, so the room cannot hold the keys): one traversal per filled slot, each finding the least key
// above the previous slot's, kept in registers.  Both then pad the rest of the room and write the full count.
template <bool SELECT>
__global__ __launch_bounds__(kCrossBlock, 8) void crossing_list_kernel(const CrossListParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kCrossBlock]
    const int32_t i = (int32_t)blockIdx.x * kCrossBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const size_t i3 = (size_t)i * 3;
    const float tmax = p.tmax ? p.tmax[i] : __int_as_float(0x7f800000);
    int spill[kMaxStack - kLdsStack];
    CrossStack stack = query_stack(lds_stack, spill, p.stack_depth);
    int32_t total = 0, filled = 0;                              // (filled <= total: int32)
    if constexpr (!SELECT) {
        xl_trace(p, stack, i3, tmax, [&](int32_t k, int32_t slot, float t, float tv, float tw, float det, int sign) {
            total++;
            size_t start;
            uint64_t room;
            xl_room(p, i, start, room);                         // (read again per pair: not held across the traversal)
            if (room == 0) return;
            int32_t tid;
            uint64_t pos;
            if ((uint64_t)filled < room) {
                pos = (uint64_t)filled++;
                tid = p.tri_id[slot];
            } else {                                            // full: enter only below the last entry
                const size_t last = start + (size_t)(room - 1);
                const float lt = p.t[last];
                if (t > lt) return;
                if (t == lt) {
                    if (k > p.instance[last]) return;           // (instances arrive in ascending order: k >= the last's)
                    tid = p.tri_id[slot];
                    if (tid > p.triangle[last]) return;
                } else {
                    tid = p.tri_id[slot];
                }
                pos = room - 1;
            }
            while (pos > 0) {                                   // shift the greater keys up by one slot
                const size_t q = start + (size_t)(pos - 1);
                const float qt = p.t[q];
                if (qt < t) break;
                if (qt == t) {
                    const int32_t qi = p.instance[q];
                    if (qi < k || (qi == k && p.triangle[q] < tid)) break;
                }
                p.t[q + 1] = qt;
                p.instance[q + 1] = p.instance[q];
                p.triangle[q + 1] = p.triangle[q];
                if (p.sign) p.sign[q + 1] = p.sign[q];
                if (p.barycentric) { p.barycentric[2 * q + 2] = p.barycentric[2 * q]; p.barycentric[2 * q + 3] = p.barycentric[2 * q + 1]; }
                if (p.uv) { p.uv[2 * q + 2] = p.uv[2 * q]; p.uv[2 * q + 3] = p.uv[2 * q + 1]; }
                if (p.point) {
                    p.point[3 * q + 3] = p.point[3 * q]; p.point[3 * q + 4] = p.point[3 * q + 1]; p.point[3 * q + 5] = p.point[3 * q + 2];
                }
                pos--;
            }
            xl_store(p, start + (size_t)pos, i, k, slot, tid, t, tv / det, tw / det, sign);
        });
    } else {
        // pass j finds the least key (t, instance, triangle) above the last one stored; pass 0 also counts.  min(count, room)
        // passes, at least one.  The winner's b1, b2 and sign come from testing its triangle again (the same sequence).
        float lt = 0.0f;
        int32_t lk = -1, ltid = -1;
        for (;;) {
            float bt = 0.0f;
            int32_t bk = -1, bslot = 0, btid = 0;
            const bool first = filled == 0 && lk < 0;
            xl_trace(p, stack, i3, tmax, [&](int32_t k, int32_t slot, float t, float, float, float, int) {
                if (first) total++;
                if (lk >= 0) {                                  // above the last key?
                    if (t < lt || (t == lt && k < lk)) return;
                    if (t == lt && k == lk && p.tri_id[slot] <= ltid) return;
                }
                if (bk >= 0 && (t > bt || (t == bt && k > bk))) return;
                const int32_t tid = p.tri_id[slot];
                if (bk >= 0 && t == bt && k == bk && tid > btid) return;
                bt = t; bk = k; bslot = slot; btid = tid;
            });
            size_t start;
            uint64_t room;
            xl_room(p, i, start, room);
            if (bk < 0 || (uint64_t)filled >= room) break;
            const DevInstance& in = p.instances[bk];
            const XqRay r = xq_ray(in, v3(p.org[i3], p.org[i3 + 1], p.org[i3 + 2]), v3(p.dir[i3], p.dir[i3 + 1], p.dir[i3 + 2]));
            const float4* rec = p.records + (size_t)bslot * 4;
            V3 a, ab, ac;
            pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
            float t = 0.0f, tv = 0.0f, tw = 0.0f, det = 1.0f;
            const int sign = xq_triangle_uvw(r, a, ab, ac, tmax, t, tv, tw, det);
            xl_store(p, start + (size_t)filled, i, bk, bslot, btid, bt, tv / det, tw / det, sign);
            filled++;
            if ((uint64_t)filled >= room || filled >= total) break;
            lt = bt; lk = bk; ltid = btid;
        }
    }
    size_t start;
    uint64_t room;
    xl_room(p, i, start, room);
    for (uint64_t j = (uint64_t)filled; j < room; j++) {        // padding
        const size_t q = start + (size_t)j;
        if (p.t) p.t[q] = __int_as_float(0x7f800000);
        if (p.instance) p.instance[q] = -1;
        if (p.triangle) p.triangle[q] = -1;
        if (p.sign) p.sign[q] = 0;
        if (p.barycentric) { p.barycentric[2 * q] = 0.0f; p.barycentric[2 * q + 1] = 0.0f; }
        if (p.uv) { p.uv[2 * q] = 0.0f; p.uv[2 * q + 1] = 0.0f; }
        if (p.point) { p.point[3 * q] = 0.0f; p.point[3 * q + 1] = 0.0f; p.point[3 * q + 2] = 0.0f; }
    }
    if (p.count) p.count[i] = total;
}

// Exclusive int64 scan for rt_crossing_offsets: out[j] = the sum of in[..j) within blocks of kScanBlock elements (in[j] = 0 for
// j >= n_in), sums[block] = the block's total.  In place is allowed (each thread reads its elements before any is written).
constexpr int kScanThreads = 256, kScanItems = 4, kScanBlock = kScanThreads * kScanItems;
template <typename T>
__global__ __launch_bounds__(kScanThreads) void scan_block_kernel(const T* in, int64_t n_in, int64_t* out, int64_t m, int64_t* sums)
{
    __shared__ long long part[kScanThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
    long long v[kScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        v[k] = base + k < n_in ? (long long)in[base + k] : 0;
        s += v[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long x = s;                                            // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) part[wave] = x;
    __syncthreads();
    long long run = x - s;
    for (int k = 0; k < wave; k++) run += part[k];
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < m) out[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == kScanThreads - 1) sums[blockIdx.x] = run;
}
__global__ __launch_bounds__(kScanThreads) void scan_add_kernel(int64_t* out, int64_t m, const int64_t* sums)
{
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
    const int64_t add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; k++)
        if (base + k < m) out[base + k] += add;
}

// ---------------------------------------------------------------------------------------------------------
// Nearby-triangle lists (rt_nearby_offsets / rt_list_nearby): every (instance, triangle) whose d2 (rules 1-3 of rt_closest_points) is
// a candidate under rule 4, in the order (d2, instance, triangle) of rule 5, written into the point's own room (include/rt_hip.h
// rule 9).  The traversal is closest_point_kernel's: the same q, pq_box_lb and pruning argument.
// ---------------------------------------------------------------------------------------------------------
struct NearbyParams {
    const float4* records;
    const float* tri_uv;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* pts;           // [n][3] world points
    const float* max_distance;  // [n] or null (= +inf)
    int32_t n;
    const int64_t* offsets;     // [n + 1] (CSR rooms) or null: fixed rooms of max_hits
    int32_t max_hits;
    float* distance;            // the keys, required by the list kernel (d2 while it runs, sqrtf(d2) at its end); indexed by room slot
    int32_t *instance, *triangle;
    float *point, *normal, *barycentric, *uv;   // optional, indexed by room slot
    int32_t *count, *pops;      // optional, [n] (the count kernel: count = the workspace)
};

// closest_point_kernel's nearest-first traversal of every instance for point i, calling leaf(k, slot, d2, b1, b2) at each triangle with
// d2 <= lim() (NaN fails).  lim() is read at every box and triangle: the list kernel lowers it while the traversal runs.  The point is
// read again at each instance, so it is not held in registers across the traversal.  Returns the interior nodes visited.
template <typename Lim, typename Leaf>
__device__ __forceinline__ int32_t nb_trace(const NearbyParams& p, PointStack& stack, size_t i3, Lim&& lim, Leaf&& leaf)
{
    int32_t pops = 0;
    for (int32_t k = 0; k < p.num_instances; k++) {
        const DevInstance& in = p.instances[k];
        const V3 q = apply_quat(in.q_pose, v3(p.pts[i3] - in.pose_xyz[0], p.pts[i3 + 1] - in.pose_xyz[1], p.pts[i3 + 2] - in.pose_xyz[2]));
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: both child boxes, nearer first
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const float la = pq_box_lb(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, q);
                const float lb = pq_box_lb(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, q);
                const float l = lim();
                const bool pa = !(prune && la > l), pb = !(prune && lb > l);      // (equality is kept: a tie may still enter)
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                const bool a_near = !(lb < la);
                if (pa && pb) stack.push(a_near ? rb : ra);
                cur = (pa && pb) ? (a_near ? ra : rb) : (pa ? ra : (pb ? rb : kNeedPop));
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    V3 a, ab, ac;
                    pq_triangle(rec[0], rec[1], rec[2], s, a, ab, ac);
                    const float2 bw = pq_weights(q, a, ab, ac);
                    const float d2 = pq_d2(q - pq_combine(a, ab, ac, bw.x, bw.y));
                    if (d2 <= lim()) leaf(k, slot, d2, bw.x, bw.y);
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel);
    }
    return pops;
}

// rt_nearby_offsets' first step: the number of pairs of each point into count (the workspace), with the fixed limit cut2
__global__ __launch_bounds__(kPointBlock, 8) void nearby_count_kernel(const NearbyParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kPointBlock]
    const int32_t i = (int32_t)blockIdx.x * kPointBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const float cut2 = pq_cut2(p.max_distance ? p.max_distance[i] : __int_as_float(0x7f800000));
    int spill[kMaxStack - kLdsStack];
    PointStack stack = query_stack(lds_stack, spill, p.stack_depth);
    int32_t total = 0;
    if (cut2 >= 0.0f)
        nb_trace(p, stack, (size_t)i * 3, [&] { return cut2; }, [&](int32_t, int32_t, float, float, float) { total++; });
    p.count[i] = total;
}

// slot j (absolute) of a room <- the pair (instance k, record slot, triangle tid) at d2 with weights (b1, b2); each optional field exactly
// as closest_point_kernel writes its winner's
__device__ __forceinline__ void nb_store(const NearbyParams& p, size_t j, int32_t k, int32_t slot, int32_t tid, float d2, float b1, float b2)
{
    p.distance[j] = d2;
    p.instance[j] = k;
    p.triangle[j] = tid;
    if (p.barycentric) { p.barycentric[2 * j] = b1; p.barycentric[2 * j + 1] = b2; }
    if (!(p.point || p.normal || p.uv)) return;
    const DevInstance& in = p.instances[k];
    if (p.point) {                                              // c again (same sequence), to world: apply_lre(inv_pose, c)
        const float4* rec = p.records + (size_t)slot * 4;
        V3 a, ab, ac;
        pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
        const V3 c = pq_combine(a, ab, ac, b1, b2);
        const V3 o = apply_quat(in.q_inv_pose, v3(c.x - in.inv_pose_xyz[0], c.y - in.inv_pose_xyz[1], c.z - in.inv_pose_xyz[2]));
        p.point[3 * j] = o.x; p.point[3 * j + 1] = o.y; p.point[3 * j + 2] = o.z;
    }
    if (p.normal) {
        const V3 nn = pq_normal(p, in, slot);
        p.normal[3 * j] = nn.x; p.normal[3 * j + 1] = nn.y; p.normal[3 * j + 2] = nn.z;
    }
    if (p.uv) {                                                 // w = (1 - b2) - b1, uv = (w uv0 + b1 uv1) + b2 uv2
        const float* t = p.tri_uv + (size_t)slot * 6;
        const float u0 = (1.0f - b2) - b1;
        p.uv[2 * j] = (u0 * t[0] + b1 * t[2]) + b2 * t[4];
        p.uv[2 * j + 1] = (u0 * t[1] + b1 * t[3]) + b2 * t[5];
    }
}

// One traversal; each pair is inserted into the point's room, which stays sorted by (d2, instance, triangle) -- lane-private, no
// atomics; once the room is full a pair enters only below the last key.  In fixed rooms without count the pruning limit then drops
// from cut2 to the last key's d2 (k-nearest): a box whose lower bound is above it holds only pairs that sort after the last key.
// Equal bounds are not pruned (a tie may still win on (instance, triangle)).  With count, or in CSR rooms, the limit stays cut2 and
// count is the full number of pairs.  distance holds d2 until the end, then sqrtf(d2) over the filled slots; the rest is padding.
__global__ __launch_bounds__(kPointBlock, 8) void nearby_list_kernel(const NearbyParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kPointBlock]
    const int32_t i = (int32_t)blockIdx.x * kPointBlock + (int32_t)threadIdx.x;     // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    const float cut2 = pq_cut2(p.max_distance ? p.max_distance[i] : __int_as_float(0x7f800000));
    int spill[kMaxStack - kLdsStack];
    PointStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const bool knn = !p.offsets && !p.count;
    float lim = cut2;
    int32_t total = 0, filled = 0, pops = 0;                    // (filled <= total: int32)
    if (cut2 >= 0.0f)
        pops = nb_trace(p, stack, (size_t)i * 3, [&] { return lim; }, [&](int32_t k, int32_t slot, float d2, float b1, float b2) {
            total++;
            size_t start;
            uint64_t room;
            xl_room(p, i, start, room);                         // (read again per pair: not held across the traversal)
            if (room == 0) return;
            int32_t tid;
            uint64_t pos;
            if ((uint64_t)filled < room) {
                pos = (uint64_t)filled++;
                tid = p.tri_id[slot];
            } else {                                            // full: enter only below the last key
                const size_t last = start + (size_t)(room - 1);
                const float ld = p.distance[last];
                if (d2 > ld) return;
                if (d2 == ld) {
                    if (k > p.instance[last]) return;           // (instances arrive in ascending order: k >= the last's)
                    tid = p.tri_id[slot];
                    if (tid > p.triangle[last]) return;
                } else {
                    tid = p.tri_id[slot];
                }
                pos = room - 1;
            }
            while (pos > 0) {                                   // shift the greater keys up by one slot
                const size_t q = start + (size_t)(pos - 1);
                const float qd = p.distance[q];
                if (qd < d2) break;
                if (qd == d2) {
                    const int32_t qi = p.instance[q];
                    if (qi < k || (qi == k && p.triangle[q] < tid)) break;
                }
                p.distance[q + 1] = qd;
                p.instance[q + 1] = p.instance[q];
                p.triangle[q + 1] = p.triangle[q];
                if (p.barycentric) { p.barycentric[2 * q + 2] = p.barycentric[2 * q]; p.barycentric[2 * q + 3] = p.barycentric[2 * q + 1]; }
                if (p.uv) { p.uv[2 * q + 2] = p.uv[2 * q]; p.uv[2 * q + 3] = p.uv[2 * q + 1]; }
                if (p.point) {
                    p.point[3 * q + 3] = p.point[3 * q]; p.point[3 * q + 4] = p.point[3 * q + 1]; p.point[3 * q + 5] = p.point[3 * q + 2];
                }
                if (p.normal) {
                    p.normal[3 * q + 3] = p.normal[3 * q]; p.normal[3 * q + 4] = p.normal[3 * q + 1]; p.normal[3 * q + 5] = p.normal[3 * q + 2];
                }
                pos--;
            }
            nb_store(p, start + (size_t)pos, k, slot, tid, d2, b1, b2);
            if (knn && (uint64_t)filled >= room) lim = p.distance[start + (size_t)(room - 1)];     // (<= cut2: only candidates enter)
        });
    size_t start;
    uint64_t room;
    xl_room(p, i, start, room);
    for (uint64_t j = 0; j < room; j++) {
        const size_t q = start + (size_t)j;
        if (j < (uint64_t)filled) {
            p.distance[q] = sqrtf(p.distance[q]);
            continue;
        }
        p.distance[q] = FLT_MAX;                                // padding: a closest-point miss
        p.instance[q] = -1;
        p.triangle[q] = -1;
        if (p.barycentric) { p.barycentric[2 * q] = 0.0f; p.barycentric[2 * q + 1] = 0.0f; }
        if (p.uv) { p.uv[2 * q] = 0.0f; p.uv[2 * q + 1] = 0.0f; }
        if (p.point) { p.point[3 * q] = 0.0f; p.point[3 * q + 1] = 0.0f; p.point[3 * q + 2] = 0.0f; }
        if (p.normal) { p.normal[3 * q] = 0.0f; p.normal[3 * q + 1] = 0.0f; p.normal[3 * q + 2] = 0.0f; }
    }
    if (p.count) p.count[i] = total;
    if (p.pops) p.pops[i] = pops;
}


// ---------------------------------------------------------------------------------------------------------
// Triangle intersections (rt_count_intersecting / rt_intersecting_offsets / rt_list_intersecting): every (instance, triangle) that a
// caller's world triangle meets by rule 10 of include/rt_hip.h -- the box pre-test, then six segment tests of rule 3 -- equal to a
// brute-force loop over every (instance, triangle) whatever the tree; the pruning argument is in DESIGN.md section 15.  One wave per
// workgroup, one query triangle per lane, an unordered traversal on the general stack: every child box that overlaps the query's
// box (widened as pq_gap widens it) is visited.
// ---------------------------------------------------------------------------------------------------------
struct TriParams {
    const float4* records;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* tris;          // [n][3][3] world query triangles
    const int32_t* skip;        // [n] or null: one instance per query whose pairs are never reported (-1 = none)
    int32_t n;
    const int64_t* offsets;     // the list kernel: [n + 1] (CSR rooms) or null: fixed rooms of max_hits
    int32_t max_hits;
    int32_t *instance, *triangle;   // the list kernel's keys, required; indexed by room slot
    float *normal, *segment;    // optional, [slots][3] and [slots][2][3]
    int32_t* count;             // optional, [n] (the offsets call: the workspace)
    uint8_t* any;               // optional, [n] (the count kernel)
    int32_t* pops;              // optional, [n]
};
constexpr int kTriBlock = 64;
typedef StackT<kTriBlock> TriStack;

// query vertex k of triangle P (world, [3][3]) in instance in's scaled mesh space: apply_lre(pose, P_k), rule 1's map
__device__ __forceinline__ V3 ti_vertex(const float* P, const DevInstance& in, int k)
{
    return apply_quat(in.q_pose, v3(P[3 * k] - in.pose_xyz[0], P[3 * k + 1] - in.pose_xyz[1], P[3 * k + 2] - in.pose_xyz[2]));
}
__device__ __forceinline__ V3 ti_min3(V3 a, V3 b, V3 c) { return v3(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z)); }
__device__ __forceinline__ V3 ti_max3(V3 a, V3 b, V3 c) { return v3(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z)); }

// One axis of a child box against the query's box: the box scaled and widened exactly as pq_gap does it; kept unless a compare says
// it lies wholly on one side, so a NaN anywhere keeps it
__device__ __forceinline__ bool ti_axis(float lo, float hi, float s, float qlo, float qhi)
{
    const float x = lo * s, y = hi * s;
    const float l = s < 0.0f ? y : x, h = s < 0.0f ? x : y;
    const float m = fmaxf(fabsf(l), fabsf(h)) * 0x1p-16f + 0x1p-126f;
    return !((l - m) > qhi) && !(qlo > (h + m));
}
__device__ __forceinline__ bool ti_box(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, V3 qlo, V3 qhi)
{
    return ti_axis(lx, hx, s.x, qlo.x, qhi.x) && ti_axis(ly, hy, s.y, qlo.y, qhi.y) && ti_axis(lz, hz, s.z, qlo.z, qhi.z);
}

// Rule 10 step 4 for one pair whose boxes overlap: the query's edges Q0->Q1, Q1->Q2, Q2->Q0 against (A, B, C), then the scene
// triangle's edges A->B, B->C, C->A against (Q0, Q1, Q2), each rule 3 with tmax = 1 on o' = X, d' = Y - X.  hit: whether one counts;
// with `all` every test runs and p0 / p1 are the mesh-space points X + t*d' of the first and the last counting test; without it the
// tests stop at the first that counts.  The query's vertices are mapped again here (the same sequence as the traversal's box), and
// the whole test is out of line, so none of it occupies the traversal's registers.
struct TiHit { int hit; V3 p0, p1; };
__device__ __noinline__ TiHit ti_segments(const float* P, const DevInstance& in, V3 a, V3 b, V3 c, bool all)
{
    const V3 q0 = ti_vertex(P, in, 0), q1 = ti_vertex(P, in, 1), q2 = ti_vertex(P, in, 2);
    TiHit h;
    h.hit = 0; h.p0 = v3(0.0f, 0.0f, 0.0f); h.p1 = h.p0;
#pragma unroll
    for (int e = 0; e < 6; e++) {
        const V3 x = e == 0 ? q0 : e == 1 ? q1 : e == 2 ? q2 : e == 3 ? a : e == 4 ? b : c;
        const V3 y = e == 0 ? q1 : e == 1 ? q2 : e == 2 ? q0 : e == 3 ? b : e == 4 ? c : a;
        const V3 d = y - x;
        XqRay r;
        xq_shear(r, x, d);
        if (r.zero) continue;                                   // (a zero d' counts nothing)
        float t = 0.0f, tv = 0.0f, tw = 0.0f, det = 0.0f;
        const int sign = e < 3 ? xq_vertices(r, a, b, c, 1.0f, t, tv, tw, det) : xq_vertices(r, q0, q1, q2, 1.0f, t, tv, tw, det);
        if (sign == 0) continue;
        const V3 pt = v3(x.x + t * d.x, x.y + t * d.y, x.z + t * d.z);
        if (!h.hit) h.p0 = pt;
        h.hit = 1;
        h.p1 = pt;
        if (!all) break;
    }
    return h;
}

// Every pair of query i, instance by instance in ascending order (triangles of one instance in tree order), skipping skip[i].
// go(k) is asked before instance k (false ends the traversal); pair(k, slot, hit) is called at each pair and returns whether to end
// the traversal.  all: whether the pair needs the segment ends.  Returns the interior nodes visited.
template <typename Go, typename Pair>
__device__ __forceinline__ int32_t ti_trace(const TriParams& p, TriStack& stack, int32_t i, bool all, Go&& go, Pair&& pair)
{
    int32_t pops = 0;
    const float* P = p.tris + (size_t)i * 9;
    const int32_t skip = p.skip ? p.skip[i] : -1;
    for (int32_t k = 0; k < p.num_instances; k++) {
        if (k == skip) continue;
        if (!go(k)) break;
        const DevInstance& in = p.instances[k];
        const V3 q0 = ti_vertex(P, in, 0), q1 = ti_vertex(P, in, 1), q2 = ti_vertex(P, in, 2);
        const V3 qlo = ti_min3(q0, q1, q2), qhi = ti_max3(q0, q1, q2);   // rule 10 step 3's box of the query
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        bool done = false;
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: every child whose box overlaps, no order
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const bool pa = !prune || ti_box(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, qlo, qhi);
                const bool pb = !prune || ti_box(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, qlo, qhi);
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                if (pa && pb) stack.push(rb);
                cur = pa ? ra : (pb ? rb : kNeedPop);
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    V3 a, ab, ac;
                    pq_triangle(rec[0], rec[1], rec[2], s, a, ab, ac);
                    const V3 b = a + ab, c = a + ac;
                    const V3 tlo = ti_min3(a, b, c), thi = ti_max3(a, b, c);
                    // step 3 first (NaN fails); the six segment tests only behind it
                    if (tlo.x <= qhi.x && qlo.x <= thi.x && tlo.y <= qhi.y && qlo.y <= thi.y && tlo.z <= qhi.z && qlo.z <= thi.z) {
                        const TiHit h = ti_segments(P, in, a, b, c, all);
                        if (h.hit && pair(k, slot, h)) done = true;
                    }
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel && !done);
        if (done) break;
    }
    return pops;
}

// ANY = false: the number of pairs of each query (rt_count_intersecting, and rt_intersecting_offsets' first step into the workspace).
// ANY = true (any wanted, count not): the traversal ends at the first pair, across instances too.
template <bool ANY>
__global__ __launch_bounds__(kTriBlock, 8) void intersect_count_kernel(const TriParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    int32_t total = 0;
    const int32_t pops = ti_trace(p, stack, i, false, [&](int32_t) { return true; }, [&](int32_t, int32_t, const TiHit&) {
        total++;
        return ANY;
    });
    if (p.count) p.count[i] = total;
    if (p.any) p.any[i] = total > 0 ? 1 : 0;
    if (p.pops) p.pops[i] = pops;
}

// The intersection half of rt_closest_to_triangles (rule 14 step 5): rule 10's pairs of the same triangles with the same skip, one
// query per lane, patching what triangle_closest_kernel wrote on the same stream -- clearance becomes 0 and within 1 where the
// triangle intersects the scene (as segment_crossing_kernel patches its three).  COUNT (intersections wanted): every pair is
// counted; otherwise the traversal ends at the first pair, and a lane whose answer cannot change any more does not traverse.
template <bool COUNT>
__global__ __launch_bounds__(kTriBlock, 8) void triangle_intersect_patch_kernel(const TriParams p, int32_t* intersections, float* clearance,
                                                                                int32_t* within)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    if (!COUNT && !clearance && within[i] != 0) return;         // (within alone, and the distance half has already said 1)
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    int32_t total = 0;
    ti_trace(p, stack, i, false, [&](int32_t) { return true; }, [&](int32_t, int32_t, const TiHit&) {
        total++;
        return !COUNT;
    });
    if (COUNT) intersections[i] = total;
    if (total > 0) {
        if (clearance) clearance[i] = 0.0f;
        if (within) within[i] = 1;
    }
}

// slot j (absolute) of a room <- the pair (instance k, record slot, triangle tid) with the segment ends h (mesh space)
__device__ __forceinline__ void ti_store(const TriParams& p, size_t j, int32_t k, int32_t slot, int32_t tid, const TiHit& h)
{
    p.instance[j] = k;
    p.triangle[j] = tid;
    if (!(p.normal || p.segment)) return;
    const DevInstance& in = p.instances[k];
    if (p.normal) {
        const V3 nn = pq_normal(p, in, slot);
        p.normal[3 * j] = nn.x; p.normal[3 * j + 1] = nn.y; p.normal[3 * j + 2] = nn.z;
    }
    if (p.segment) {                                            // to world: apply_lre(inv_pose, .), closest_points' map
        const V3 w0 = apply_quat(in.q_inv_pose, v3(h.p0.x - in.inv_pose_xyz[0], h.p0.y - in.inv_pose_xyz[1], h.p0.z - in.inv_pose_xyz[2]));
        const V3 w1 = apply_quat(in.q_inv_pose, v3(h.p1.x - in.inv_pose_xyz[0], h.p1.y - in.inv_pose_xyz[1], h.p1.z - in.inv_pose_xyz[2]));
        float* o = p.segment + 6 * j;
        o[0] = w0.x; o[1] = w0.y; o[2] = w0.z; o[3] = w1.x; o[4] = w1.y; o[5] = w1.z;
    }
}

// One traversal; each pair is inserted into the query's room, which stays sorted by (instance, triangle) -- lane-private, no atomics.
// Pairs arrive instance by instance in ascending order, so only the order within an instance needs the insertion (tree order is not
// triangle order).  Once the room is full a pair enters only below the last key.  In fixed rooms without count the traversal then
// ends after the last key's instance: every later pair sorts after it.  Within that instance nothing can be skipped (triangle indices
// are not spatial).  The rooms are the same bits with and without count.
__global__ __launch_bounds__(kTriBlock, 8) void intersect_list_kernel(const TriParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const bool early = !p.offsets && !p.count;
    int32_t total = 0, filled = 0;                              // (filled <= total: int32)
    const int32_t pops = ti_trace(p, stack, i, p.segment != nullptr, [&](int32_t k) {
        if (!early || filled < p.max_hits) return true;         // (fixed rooms: start i*K, room K)
        return k <= p.instance[(size_t)i * (size_t)p.max_hits + (size_t)(p.max_hits - 1)];
    }, [&](int32_t k, int32_t slot, const TiHit& h) {
        total++;
        size_t start;
        uint64_t room;
        xl_room(p, i, start, room);                             // (read again per pair: not held across the traversal)
        if (room == 0) return false;
        const int32_t tid = p.tri_id[slot];
        uint64_t pos;
        if ((uint64_t)filled < room) {
            pos = (uint64_t)filled++;
        } else {                                                // full: enter only below the last key
            const size_t last = start + (size_t)(room - 1);
            const int32_t li = p.instance[last];
            if (k > li || (k == li && tid > p.triangle[last])) return false;      // (instances arrive in ascending order: k >= li)
            pos = room - 1;
        }
        while (pos > 0) {                                       // shift the greater keys of this instance up by one slot
            const size_t q = start + (size_t)(pos - 1);
            const int32_t qi = p.instance[q];
            if (qi < k || p.triangle[q] < tid) break;           // (qi <= k: an earlier instance, or this one below tid)
            p.instance[q + 1] = qi;
            p.triangle[q + 1] = p.triangle[q];
            if (p.normal) { p.normal[3 * q + 3] = p.normal[3 * q]; p.normal[3 * q + 4] = p.normal[3 * q + 1]; p.normal[3 * q + 5] = p.normal[3 * q + 2]; }
            if (p.segment) {
                for (int c = 0; c < 6; c++) p.segment[6 * q + 6 + c] = p.segment[6 * q + c];
            }
            pos--;
        }
        ti_store(p, start + (size_t)pos, k, slot, tid, h);
        return false;
    });
    size_t start;
    uint64_t room;
    xl_room(p, i, start, room);
    for (uint64_t j = (uint64_t)filled; j < room; j++) {        // padding
        const size_t q = start + (size_t)j;
        p.instance[q] = -1;
        p.triangle[q] = -1;
        if (p.normal) { p.normal[3 * q] = 0.0f; p.normal[3 * q + 1] = 0.0f; p.normal[3 * q + 2] = 0.0f; }
        if (p.segment) { for (int c = 0; c < 6; c++) p.segment[6 * q + c] = 0.0f; }
    }
    if (p.count) p.count[i] = total;
    if (p.pops) p.pops[i] = pops;
}


// ---------------------------------------------------------------------------------------------------------
// Box queries (rt_count_in_boxes / rt_box_offsets / rt_list_in_boxes / rt_occupancy_grid): every (instance, triangle) that meets a
// caller's world axis-aligned box by rule 11 of include/rt_hip.h -- the box pre-test, then thirteen separating axes relative to the
// box's first corner -- equal to a brute-force loop over every (instance, triangle) whatever the tree; the pruning argument is in
// DESIGN.md section 16.  One wave per workgroup, one box per lane, the intersecting triangles' unordered traversal on the general
// stack: every child box that overlaps the mapped box's bounds (widened as pq_gap widens it) is visited.
// ---------------------------------------------------------------------------------------------------------
struct BoxParams {
    const float4* records;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* boxes;         // [n][2][3] world boxes, lo then hi (the grid kernel makes its own)
    int32_t n;
    const int64_t* offsets;     // the list kernel: [n + 1] (CSR rooms) or null: fixed rooms of max_hits
    int32_t max_hits;
    int32_t *instance, *triangle;   // the list kernel's keys, required; indexed by room slot
    int32_t* count;             // optional, [n] (the offsets call: the workspace)
    uint8_t* any;               // optional, [n] (the count and the grid kernel)
    int32_t* pops;              // optional, [n]
    float origin[3], spacing[3];    // the grid kernel: cell (ix, iy, iz) is origin + i*spacing .. origin + (i + 1)*spacing
    int32_t dims[3];            // nx, ny, nz
    uint32_t bricks[3];         // 4x4x4 bricks per axis
};

// corner k of the world box lo..hi (bit a of k set: hi on axis a) in instance in's scaled mesh space: apply_lre(pose, corner)
__device__ __forceinline__ V3 bx_corner(V3 lo, V3 hi, const DevInstance& in, int k)
{
    return apply_quat(in.q_pose, v3(((k & 1) ? hi.x : lo.x) - in.pose_xyz[0], ((k & 2) ? hi.y : lo.y) - in.pose_xyz[1],
                                    ((k & 4) ? hi.z : lo.z) - in.pose_xyz[2]));
}
__device__ __forceinline__ float bx_dot(V3 a, V3 x) { return (a.x * x.x + a.y * x.y) + a.z * x.z; }
__device__ __forceinline__ V3 bx_cross(V3 u, V3 v) { return v3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }

// one axis of rule 11 step 5: whether it separates the box (corners r[0..7] relative to C0) from the triangle (ta, tb, tc); a zero
// axis gives two intervals [0, 0], a NaN fails both compares: neither separates
__device__ __forceinline__ bool bx_separates(V3 ax, const V3* r, V3 ta, V3 tb, V3 tc)
{
    float minb = bx_dot(ax, r[0]), maxb = minb;
#pragma unroll
    for (int k = 1; k < 8; k++) {
        const float d = bx_dot(ax, r[k]);
        minb = fminf(minb, d); maxb = fmaxf(maxb, d);
    }
    const float da = bx_dot(ax, ta), db = bx_dot(ax, tb), dc = bx_dot(ax, tc);
    const float mint = fminf(fminf(da, db), dc), maxt = fmaxf(fmaxf(da, db), dc);
    return maxt < minb || maxb < mint;
}

// Rule 11 steps 2, 3 and 5 for one pair that passed step 4: true when no axis separates.  The corners are mapped again here (the same
// sequence as the traversal's bounds), and the whole test is out of line, so none of it occupies the traversal's registers.
__device__ __noinline__ bool bx_axes(V3 lo, V3 hi, const DevInstance& in, V3 a, V3 b, V3 c)
{
    const V3 c0 = bx_corner(lo, hi, in, 0);
    V3 r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = bx_corner(lo, hi, in, k) - c0;
    const V3 ta = a - c0, tb = b - c0, tc = c - c0;
    const V3 f0 = b - a, f1 = c - b, f2 = a - c;
    if (bx_separates(r[1], r, ta, tb, tc) || bx_separates(r[2], r, ta, tb, tc) || bx_separates(r[4], r, ta, tb, tc)) return false;
    if (bx_separates(bx_cross(f0, f1), r, ta, tb, tc)) return false;
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const V3 e = r[1 << m];
        if (bx_separates(bx_cross(e, f0), r, ta, tb, tc) || bx_separates(bx_cross(e, f1), r, ta, tb, tc) ||
            bx_separates(bx_cross(e, f2), r, ta, tb, tc))
            return false;
    }
    return true;
}

// Every pair of the world box lo..hi, instance by instance in ascending order (triangles of one instance in tree order).  go(k) is
// asked before instance k (false ends the traversal); pair(k, slot) is called at each pair and returns whether to end the traversal.
// Returns the interior nodes visited.  An invalid box (an inverted axis or a NaN, rule 11 step 1) visits nothing.
template <typename Go, typename Pair>
__device__ __forceinline__ int32_t bx_trace(const BoxParams& p, TriStack& stack, V3 lo, V3 hi, Go&& go, Pair&& pair)
{
    int32_t pops = 0;
    if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) return pops;
    for (int32_t k = 0; k < p.num_instances; k++) {
        if (!go(k)) break;
        const DevInstance& in = p.instances[k];
        V3 qlo = bx_corner(lo, hi, in, 0), qhi = qlo;           // rule 11 step 4's bounds of the mapped box: the chain over C0..C7
#pragma unroll
        for (int c = 1; c < 8; c++) {
            const V3 q = bx_corner(lo, hi, in, c);
            qlo = v3(fminf(qlo.x, q.x), fminf(qlo.y, q.y), fminf(qlo.z, q.z));
            qhi = v3(fmaxf(qhi.x, q.x), fmaxf(qhi.y, q.y), fmaxf(qhi.z, q.z));
        }
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        bool done = false;
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: every child whose box overlaps, no order
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                const bool pa = !prune || ti_box(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, qlo, qhi);
                const bool pb = !prune || ti_box(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, qlo, qhi);
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                if (pa && pb) stack.push(rb);
                cur = pa ? ra : (pb ? rb : kNeedPop);
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    V3 a, ab, ac;
                    pq_triangle(rec[0], rec[1], rec[2], s, a, ab, ac);
                    const V3 b = a + ab, c = a + ac;
                    const V3 tlo = ti_min3(a, b, c), thi = ti_max3(a, b, c);
                    // step 4 first (NaN fails); the thirteen axes only behind it
                    if (tlo.x <= qhi.x && qlo.x <= thi.x && tlo.y <= qhi.y && qlo.y <= thi.y && tlo.z <= qhi.z && qlo.z <= thi.z) {
                        if (bx_axes(lo, hi, in, a, b, c) && pair(k, slot)) done = true;
                    }
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel && !done);
        if (done) break;
    }
    return pops;
}

// ANY = false: the number of pairs of each box (rt_count_in_boxes, and rt_box_offsets' first step into the workspace).
// ANY = true (any wanted, count not): the traversal ends at the first pair, across instances too.
template <bool ANY>
__global__ __launch_bounds__(kTriBlock, 8) void box_count_kernel(const BoxParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const float* B = p.boxes + (size_t)i * 6;
    int32_t total = 0;
    const int32_t pops = bx_trace(p, stack, v3(B[0], B[1], B[2]), v3(B[3], B[4], B[5]), [&](int32_t) { return true; },
                                  [&](int32_t, int32_t) {
        total++;
        return ANY;
    });
    if (p.count) p.count[i] = total;
    if (p.any) p.any[i] = total > 0 ? 1 : 0;
    if (p.pops) p.pops[i] = pops;
}

// The count kernel on the cells of a grid, which it makes itself: a wave takes a 4x4x4 brick of cells (lane = x + 4y + 16z within the
// brick), so its lanes walk the same part of the tree; lanes outside a partial brick do nothing.  Cell bounds are origin + (float)i *
// spacing (the product rounded, then the sum), so neighbouring cells share their faces bit for bit.  Outputs [nz][ny][nx].
template <bool ANY>
__global__ __launch_bounds__(kTriBlock, 8) void box_grid_kernel(const BoxParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const uint32_t brick = blockIdx.y * gridDim.x + blockIdx.x;                     // (bricks <= cells <= INT32_MAX)
    if (brick >= p.bricks[0] * p.bricks[1] * p.bricks[2]) return;
    const uint32_t t = threadIdx.x, bxy = brick / p.bricks[0];
    const int32_t ix = (int32_t)((brick - bxy * p.bricks[0]) * 4u + (t & 3u));
    const int32_t iy = (int32_t)((bxy % p.bricks[1]) * 4u + ((t >> 2) & 3u));
    const int32_t iz = (int32_t)((bxy / p.bricks[1]) * 4u + (t >> 4));
    if (ix >= p.dims[0] || iy >= p.dims[1] || iz >= p.dims[2]) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const V3 lo = v3(p.origin[0] + (float)ix * p.spacing[0], p.origin[1] + (float)iy * p.spacing[1], p.origin[2] + (float)iz * p.spacing[2]);
    const V3 hi = v3(p.origin[0] + (float)(ix + 1) * p.spacing[0], p.origin[1] + (float)(iy + 1) * p.spacing[1],
                     p.origin[2] + (float)(iz + 1) * p.spacing[2]);
    int32_t total = 0;
    bx_trace(p, stack, lo, hi, [&](int32_t) { return true; }, [&](int32_t, int32_t) {
        total++;
        return ANY;
    });
    const size_t cell = ((size_t)iz * (size_t)p.dims[1] + (size_t)iy) * (size_t)p.dims[0] + (size_t)ix;   // (< cells <= INT32_MAX)
    if (p.count) p.count[cell] = total;
    if (p.any) p.any[cell] = total > 0 ? 1 : 0;
}

// A box room's entry is its key alone: the (instance, triangle) of slot q
struct BxItem { uint64_t key; };
struct BxRoom {
    const BoxParams& p;
    __device__ __forceinline__ BxItem get(size_t q) const { return {pair_key(p.instance[q], p.triangle[q])}; }
    __device__ __forceinline__ void put(size_t q, BxItem it) const
    {
        p.instance[q] = (int32_t)(it.key >> 32);
        p.triangle[q] = (int32_t)(uint32_t)it.key;
    }
};

// One traversal; the room is kept as the room heap of its keys (instance, triangle) while pairs arrive -- lane-private, no atomics --
// and sorted in place at the end.  A box holds a volume's worth of triangles, so its lists are long where a query triangle's are
// short: the heap takes a pair in O(log room) where intersect_list_kernel's shifting insertion takes O(room).  In fixed rooms
// without count the traversal ends after the root's instance once the room is full: every later pair sorts after it (instances
// arrive in ascending order).  Which keys stay does not depend on the order of arrival, so the rooms are the same bits with and
// without count and whatever the tree.
__global__ __launch_bounds__(kTriBlock, 8) void box_list_kernel(const BoxParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const float* B = p.boxes + (size_t)i * 6;
    const bool early = !p.offsets && !p.count;
    int32_t total = 0;
    uint64_t filled = 0;                                        // (<= room)
    const int32_t pops = bx_trace(p, stack, v3(B[0], B[1], B[2]), v3(B[3], B[4], B[5]), [&](int32_t k) {
        if (!early || filled < (uint64_t)p.max_hits) return true;                   // (fixed rooms: start i*K, room K)
        return k <= p.instance[(size_t)i * (size_t)p.max_hits];                     // (the root: the room's greatest key)
    }, [&](int32_t k, int32_t slot) {
        total++;
        size_t start;
        uint64_t room;
        xl_room(p, i, start, room);                             // (read again per pair: not held across the traversal)
        if (room == 0) return false;
        room_insert(BxRoom{p}, start, room, filled, BxItem{pair_key(k, p.tri_id[slot])});
        return false;
    });
    size_t start;
    uint64_t room;
    xl_room(p, i, start, room);
    room_sort(BxRoom{p}, start, filled);
    for (uint64_t j = filled; j < room; j++) {                  // padding
        p.instance[start + (size_t)j] = -1;
        p.triangle[start + (size_t)j] = -1;
    }
    if (p.count) p.count[i] = total;
    if (p.pops) p.pops[i] = pops;
}


// ---------------------------------------------------------------------------------------------------------
// Plane sections (rt_count_sections / rt_section_offsets / rt_list_sections): every (instance, triangle) that a caller's world plane
// cuts by rule 12 of include/rt_hip.h -- a vertex ABOVE (h >= 0) and a vertex BELOW (h < 0) -- with the oriented segment of the cut,
// equal to a brute-force loop over every (instance, triangle) whatever the tree; the pruning argument is in DESIGN.md section 17.  One
// wave per workgroup, one plane per lane, the boxes' unordered traversal on the general stack: a child box is skipped only when every
// vertex that can lie in it gets the same class.
// ---------------------------------------------------------------------------------------------------------
struct SecParams {
    const float4* records;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* planes;        // [n][2][3] world planes, point then normal
    int32_t n;
    const int64_t* offsets;     // the list kernel: [n + 1] (CSR rooms) or null: fixed rooms of max_hits
    int32_t max_hits;
    int32_t *instance, *triangle;   // the list kernel's keys, required; indexed by room slot
    float *segment, *normal;    // optional, [slots][2][3] and [slots][3]
    int32_t* count;             // optional, [n] (the offsets call: the workspace)
    uint8_t* any;               // optional, [n] (the count kernel)
    int32_t* pops;              // optional, [n]
};

// rule 12 step 2: the plane's point and normal in instance in's scaled mesh space
__device__ __forceinline__ V3 sc_point(V3 P, const DevInstance& in)
{
    return apply_quat(in.q_pose, v3(P.x - in.pose_xyz[0], P.y - in.pose_xyz[1], P.z - in.pose_xyz[2]));
}
__device__ __forceinline__ V3 sc_normal(V3 N, const DevInstance& in) { return apply_quat(in.q_pose, N); }
// rule 12 step 4: each difference rounded, each product rounded, then the two sums
__device__ __forceinline__ float sc_height(V3 n, V3 q, V3 x) { return (n.x * (x.x - q.x) + n.y * (x.y - q.y)) + n.z * (x.z - q.z); }

// One axis of a child box: the box scaled and widened exactly as pq_gap does it, then the smaller and the larger of the term
// n*(X - q) of step 4 at its two ends, and the sum of their magnitudes (>= the larger magnitude; a NaN in either end stays a NaN
// here, where fminf / fmaxf would drop it)
__device__ __forceinline__ void sc_axis(float lo, float hi, float s, float q, float n, float& lower, float& upper, float& mag)
{
    const float x = lo * s, y = hi * s;
    const float l = s < 0.0f ? y : x, h = s < 0.0f ? x : y;
    const float m = fmaxf(fabsf(l), fabsf(h)) * 0x1p-16f + 0x1p-126f;
    const float t1 = n * ((l - m) - q), t2 = n * ((h + m) - q);
    lower = fminf(t1, t2); upper = fmaxf(t1, t2); mag = fabsf(t1) + fabsf(t2);
}
// Whether a child box can hold a vertex of either class: step 4's height bounded from both sides in step 4's own order of sums,
// the bounds widened by E = 2^-16 of the terms' magnitudes plus FLT_MIN; skipped only when a compare says that every height is > 0 or
// every height is < 0, so a NaN anywhere keeps the box.  sc_bounds is the arithmetic, shared by the section and the region kernels.
__device__ __forceinline__ void sc_bounds(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, V3 q, V3 n, float& lower,
                                          float& upper, float& e)
{
    float ax, bx, mx, ay, by, my, az, bz, mz;
    sc_axis(lx, hx, s.x, q.x, n.x, ax, bx, mx);
    sc_axis(ly, hy, s.y, q.y, n.y, ay, by, my);
    sc_axis(lz, hz, s.z, q.z, n.z, az, bz, mz);
    lower = (ax + ay) + az; upper = (bx + by) + bz; e = ((mx + my) + mz) * 0x1p-16f + 0x1p-126f;
}
__device__ __forceinline__ bool sc_box(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, V3 q, V3 n)
{
    float lower, upper, e;
    sc_bounds(lx, ly, lz, hx, hy, hz, s, q, n, lower, upper, e);
    return !((lower - e) > 0.0f) && !((upper + e) < 0.0f);
}
// The upper half alone (rule 15): false when a compare says that every vertex that can lie in the box is BELOW
// the plane; a NaN keeps the box
__device__ __forceinline__ bool sc_box_above(float lx, float ly, float lz, float hx, float hy, float hz, V3 s, V3 q, V3 n)
{
    float lower, upper, e;
    sc_bounds(lx, ly, lz, hx, hy, hz, s, q, n, lower, upper, e);
    return !((upper + e) < 0.0f);
}

// Rule 12 step 6 for one pair, out of line and from the record again (the same sequence as the traversal's test, the same bits), so none
// of it occupies the traversal's registers: the two cut points in WORLD space, end 0 on the edge the cycle A->B->C->A runs from ABOVE to
// BELOW, end 1 on the edge it runs from BELOW to ABOVE, each computed from the edge's BELOW vertex.
struct ScSeg { V3 e0, e1; };
__device__ __noinline__ ScSeg sc_segment(const float4* records, const DevInstance& in, int32_t slot, V3 P, V3 N)
{
    const V3 q = sc_point(P, in), n = sc_normal(N, in);
    const float4* rec = records + (size_t)slot * 4;
    V3 a, ab, ac;
    pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
    const V3 b = a + ab, c = a + ac;
    const float ha = sc_height(n, q, a), hb = sc_height(n, q, b), hc = sc_height(n, q, c);
    ScSeg r;
    r.e0 = v3(0.0f, 0.0f, 0.0f); r.e1 = r.e0;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const V3 x = e == 0 ? a : e == 1 ? b : c, y = e == 0 ? b : e == 1 ? c : a;      // the cycle's edge x -> y
        const float hx = e == 0 ? ha : e == 1 ? hb : hc, hy = e == 0 ? hb : e == 1 ? hc : ha;
        const bool down = hx >= 0.0f && hy < 0.0f, up = hx < 0.0f && hy >= 0.0f;
        if (!(down || up)) continue;
        const V3 lo = up ? x : y, hi = up ? y : x;              // the BELOW and the ABOVE end
        const float hl = up ? hx : hy, hh = up ? hy : hx;
        const float t = hl / (hl - hh);
        const V3 cut = v3(lo.x + t * (hi.x - lo.x), lo.y + t * (hi.y - lo.y), lo.z + t * (hi.z - lo.z));
        // to world: apply_lre(inv_pose, .), closest_points' map
        const V3 w = apply_quat(in.q_inv_pose, v3(cut.x - in.inv_pose_xyz[0], cut.y - in.inv_pose_xyz[1], cut.z - in.inv_pose_xyz[2]));
        if (down) r.e0 = w; else r.e1 = w;
    }
    return r;
}

// Every pair of the world plane (P, N), instance by instance in ascending order (triangles of one instance in tree order).  go(k) is
// asked before instance k (false ends the traversal); pair(k, slot) is called at each pair and returns whether to end the traversal.
// Returns the interior nodes visited.  A zero normal (rule 12 step 1) visits nothing.
template <typename Go, typename Pair>
__device__ __forceinline__ int32_t sc_trace(const SecParams& p, TriStack& stack, V3 P, V3 N, Go&& go, Pair&& pair)
{
    int32_t pops = 0;
    if (!(N.x != 0.0f || N.y != 0.0f || N.z != 0.0f)) return pops;
    for (int32_t k = 0; k < p.num_instances; k++) {
        if (!go(k)) break;
        const DevInstance& in = p.instances[k];
        const V3 q = sc_point(P, in), n = sc_normal(N, in);     // p' and n': all the node loop keeps of the plane
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        // the child boxes that can hold both classes
        const bool done = walk_unordered(p, stack, in, boxes_ordered(p, in), pops,
                                         [&](float lx, float ly, float lz, float hx, float hy, float hz) {
            return sc_box(lx, ly, lz, hx, hy, hz, s, q, n);
        }, [&](int32_t slot, float4 t0, float4 t1, float4 t2) {
            V3 a, ab, ac;
            pq_triangle(t0, t1, t2, s, a, ab, ac);
            const float ha = sc_height(n, q, a), hb = sc_height(n, q, a + ab), hc = sc_height(n, q, a + ac);
            const int above = (ha >= 0.0f) + (hb >= 0.0f) + (hc >= 0.0f), below = (ha < 0.0f) + (hb < 0.0f) + (hc < 0.0f);
            // step 5: all three classified (a NaN height is neither), one ABOVE at least and one BELOW
            return above + below == 3 && above > 0 && below > 0 && pair(k, slot);
        });
        if (done) break;
    }
    return pops;
}

// ANY = false: the number of pairs of each plane (rt_count_sections, and rt_section_offsets' first step into the workspace).
// ANY = true (any wanted, count not): the traversal ends at the first pair, across instances too.
template <bool ANY>
__global__ __launch_bounds__(kTriBlock, 8) void section_count_kernel(const SecParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const float* B = p.planes + (size_t)i * 6;
    int32_t total = 0;
    const int32_t pops = sc_trace(p, stack, v3(B[0], B[1], B[2]), v3(B[3], B[4], B[5]), [&](int32_t) { return true; },
                                  [&](int32_t, int32_t) {
        total++;
        return ANY;
    });
    if (p.count) p.count[i] = total;
    if (p.any) p.any[i] = total > 0 ? 1 : 0;
    if (p.pops) p.pops[i] = pops;
}

// A room's entry while the heap is at work: the key (instance, triangle) as one number and the pair's record slot, which travels
// with the key when segment or normal is wanted: they are computed from it once the room is sorted.  The slot lives in the first
// word of the entry's segment (or, without segment, of its normal), inside the room.
struct ScItem { uint64_t key; int32_t slot; };
struct ScRoom {
    const SecParams& p;
    __device__ __forceinline__ float* aux(size_t q) const { return p.segment ? p.segment + 6 * q : (p.normal ? p.normal + 3 * q : nullptr); }
    __device__ __forceinline__ ScItem get(size_t q) const
    {
        ScItem it;
        it.key = pair_key(p.instance[q], p.triangle[q]);
        const float* x = aux(q);
        it.slot = x ? __float_as_int(*x) : 0;
        return it;
    }
    __device__ __forceinline__ void put(size_t q, ScItem it) const
    {
        p.instance[q] = (int32_t)(it.key >> 32);
        p.triangle[q] = (int32_t)(uint32_t)it.key;
        float* x = aux(q);
        if (x) *x = __int_as_float(it.slot);
    }
};

// box_list_kernel's room heap on (instance, triangle) and its early end for fixed rooms without count.  segment and normal
// depend on the plane, the instance and the record alone, and are written after the sort from the slot that travelled with each key:
// the rooms are the same bits with and without count and whatever the tree.
__global__ __launch_bounds__(kTriBlock, 8) void section_list_kernel(const SecParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const float* B = p.planes + (size_t)i * 6;
    const bool early = !p.offsets && !p.count;
    int32_t total = 0;
    uint64_t filled = 0;                                        // (<= room)
    const int32_t pops = sc_trace(p, stack, v3(B[0], B[1], B[2]), v3(B[3], B[4], B[5]), [&](int32_t k) {
        if (!early || filled < (uint64_t)p.max_hits) return true;                   // (fixed rooms: start i*K, room K)
        return k <= p.instance[(size_t)i * (size_t)p.max_hits];                     // (the root: the room's greatest key)
    }, [&](int32_t k, int32_t slot) {
        total++;
        size_t start;
        uint64_t room;
        xl_room(p, i, start, room);                             // (read again per pair: not held across the traversal)
        if (room == 0) return false;
        room_insert(ScRoom{p}, start, room, filled, ScItem{pair_key(k, p.tri_id[slot]), slot});
        return false;
    });
    size_t start;
    uint64_t room;
    xl_room(p, i, start, room);
    room_sort(ScRoom{p}, start, filled);
    if (p.segment || p.normal) {
        const V3 P = v3(B[0], B[1], B[2]), N = v3(B[3], B[4], B[5]);
        for (uint64_t j = 0; j < filled; j++) {                 // the sorted entries: segment and normal from the slot
            const size_t q = start + (size_t)j;
            const int32_t slot = ScRoom{p}.get(q).slot;
            const DevInstance& in = p.instances[p.instance[q]];
            if (p.segment) {
                const ScSeg sg = sc_segment(p.records, in, slot, P, N);
                float* o = p.segment + 6 * q;
                o[0] = sg.e0.x; o[1] = sg.e0.y; o[2] = sg.e0.z; o[3] = sg.e1.x; o[4] = sg.e1.y; o[5] = sg.e1.z;
            }
            if (p.normal) {
                const V3 nn = pq_normal(p, in, slot);
                p.normal[3 * q] = nn.x; p.normal[3 * q + 1] = nn.y; p.normal[3 * q + 2] = nn.z;
            }
        }
    }
    for (uint64_t j = filled; j < room; j++) {                  // padding
        const size_t q = start + (size_t)j;
        p.instance[q] = -1;
        p.triangle[q] = -1;
        if (p.segment) { for (int c = 0; c < 6; c++) p.segment[6 * q + c] = 0.0f; }
        if (p.normal) { p.normal[3 * q] = 0.0f; p.normal[3 * q + 1] = 0.0f; p.normal[3 * q + 2] = 0.0f; }
    }
    if (p.count) p.count[i] = total;
    if (p.pops) p.pops[i] = pops;
}


// ---------------------------------------------------------------------------------------------------------
// Region queries (rt_count_in_regions / rt_region_offsets / rt_list_in_regions): every (instance, triangle) that lies in or touches
// a caller's convex region -- the intersection of K half-spaces, K <= RT_REGION_MAX_PLANES, one K per call -- by rule 15 of
// include/rt_hip.h: rule 12's classes on every plane, then the triangle clipped by the planes in order; equal to a brute-force loop
// over every (instance, triangle) whatever the tree.  The pruning argument is in DESIGN.md section 20.  One wave per workgroup, one
// region per lane, the sections' traversal on the general stack: a child box is skipped when on some plane every vertex that can lie
// in it is BELOW.  The mapped planes (p'_k, n'_k: 6K words) live in registers through the node loop; the kernels are templated on a
// plane capacity KT >= K, and the call's K bounds every plane loop, so no plane is padded.
// ---------------------------------------------------------------------------------------------------------
constexpr int kRegionMaxPlanes = RT_REGION_MAX_PLANES;
constexpr int kRegionMaxVerts = 3 + kRegionMaxPlanes;
struct RegParams {
    const float4* records;
    const int32_t* tri_id;
    const int32_t* leaf_count;
    const int32_t* mesh_flags;
    const DevInstance* instances;
    int32_t num_instances;
    int32_t stack_depth;
    const float* regions;       // [n][planes][2][3] world planes, point then inward normal
    int32_t n;
    int32_t planes;             // K, 1..kRegionMaxPlanes
    const int64_t* offsets;     // the list kernel: [n + 1] (CSR rooms) or null: fixed rooms of max_hits
    int32_t max_hits;
    int32_t *instance, *triangle;   // the list kernel's keys, required; indexed by room slot
    uint8_t* flag;              // the list kernel: optional, [slots] the pair's inside flag
    float* normal;              // the list kernel: optional, [slots][3]
    int32_t* count;             // optional, [n] (the offsets call: the workspace)
    int32_t* inside;            // optional, [n] the number of wholly-inside pairs (the count kernel)
    uint8_t* any;               // optional, [n] (the count kernel)
    int32_t* pops;              // optional, [n]
};

__device__ __forceinline__ V3 rg_load(const float* R, int j) { return v3(R[3 * j], R[3 * j + 1], R[3 * j + 2]); }

// Rule 15 step 5 for one triangle that passed step 3 and is not wholly inside: whether the clip leaves a polygon.  Out of line and
// from the record and the region again (the same sequence as the traversal's heights, the same bits), so none of it occupies the
// traversal's registers; the two polygons live in scratch, which only triangles that straddle a face pay for.  A plane that has every
// current vertex above reproduces the polygon and is skipped.
__device__ __noinline__ bool rg_clip(const float4* records, const DevInstance& in, int32_t slot, const float* R, int32_t K)
{
    const float4* rec = records + (size_t)slot * 4;
    V3 a, ab, ac;
    pq_triangle(rec[0], rec[1], rec[2], v3(in.scale[0], in.scale[1], in.scale[2]), a, ab, ac);
    V3 poly[2][kRegionMaxVerts];
    float g[kRegionMaxVerts];
    poly[0][0] = a; poly[0][1] = a + ab; poly[0][2] = a + ac;
    int m = 3, cur = 0;
    for (int32_t j = 0; j < K; j++) {
        const V3 q = sc_point(rg_load(R, 2 * j), in), n = sc_normal(rg_load(R, 2 * j + 1), in);
        const V3* v = poly[cur];
        V3* w = poly[cur ^ 1];
        bool all = true;
        for (int i = 0; i < m; i++) {
            g[i] = sc_height(n, q, v[i]);
            all = all && g[i] >= 0.0f;
        }
        if (all) continue;
        int o = 0;
        for (int i = 0; i < m; i++) {
            const int i1 = i + 1 == m ? 0 : i + 1;
            const bool ai = g[i] >= 0.0f, an = g[i1] >= 0.0f;
            if (ai && o < kRegionMaxVerts) w[o++] = v[i];
            if (ai != an && o < kRegionMaxVerts) {              // the cut, from the end that is not above towards the end that is
                const V3 x = ai ? v[i1] : v[i], y = ai ? v[i] : v[i1];
                const float hx = ai ? g[i1] : g[i], hy = ai ? g[i] : g[i1];
                const float t = hx / (hx - hy);
                w[o++] = v3(x.x + t * (y.x - x.x), x.y + t * (y.y - x.y), x.z + t * (y.z - x.z));
            }
        }
        if (o == 0) return false;
        m = o; cur ^= 1;
    }
    return true;
}

// Every pair of the world region R ([K][2][3]), instance by instance in ascending order (triangles of one instance in tree order).
// go(k) is asked before instance k (false ends the traversal); pair(k, slot, inside) is called at each pair and returns whether to end
// the traversal.  Returns the interior nodes visited.  A region with a zero normal (rule 15 step 1) visits nothing.
template <int KT, typename Go, typename Pair>
__device__ __forceinline__ int32_t rg_trace(const RegParams& p, TriStack& stack, const float* R, Go&& go, Pair&& pair)
{
    int32_t pops = 0;
    const int32_t K = p.planes;                                 // (1 <= K <= KT: the C-ABI chooses KT)
#pragma unroll
    for (int j = 0; j < KT; j++) {
        if (j >= K) break;
        const V3 N = rg_load(R, 2 * j + 1);
        if (!(N.x != 0.0f || N.y != 0.0f || N.z != 0.0f)) return pops;
    }
    for (int32_t k = 0; k < p.num_instances; k++) {
        if (!go(k)) break;
        const DevInstance& in = p.instances[k];
        V3 q[KT], n[KT];                                        // p'_j and n'_j: all the node loop keeps of the region, in registers
#pragma unroll
        for (int j = 0; j < KT; j++) {
            q[j] = v3(0.0f, 0.0f, 0.0f); n[j] = q[j];
            if (j < K) { q[j] = sc_point(rg_load(R, 2 * j), in); n[j] = sc_normal(rg_load(R, 2 * j + 1), in); }
        }
        const V3 s = v3(in.scale[0], in.scale[1], in.scale[2]);
        const bool prune = (p.mesh_flags[in.mesh_index] & kBoxUnordered) == 0;      // (unordered / NaN boxes: no pruning in this mesh)
        bool done = false;
        stack.sp = 0;
        stack.push(kSentinel);
        int32_t cur = in.root_ref, rem = -1;
        do {
            if (cur >= 0) {                                     // interior node: every child that no plane has wholly below it
                pops++;
                const float4* rec = p.records + (size_t)cur * 4;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                bool pa = true, pb = true;
                if (prune) {
#pragma unroll
                    for (int j = 0; j < KT; j++) {              // left at the first plane that skips the box
                        if (j >= K || !pa) break;
                        pa = sc_box_above(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, s, q[j], n[j]);
                    }
#pragma unroll
                    for (int j = 0; j < KT; j++) {
                        if (j >= K || !pb) break;
                        pb = sc_box_above(r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, s, q[j], n[j]);
                    }
                }
                const int32_t ra = __float_as_int(r3.x), rb = __float_as_int(r3.y);
                if (pa && pb) stack.push(rb);
                cur = pa ? ra : (pb ? rb : kNeedPop);
            } else {                                            // one triangle of a leaf per iteration
                const int32_t slot = cur & kSlotMask;
                if (rem < 0) {
                    rem = (cur >> kSlotBits) & 31;
                    if (rem == 31) rem = p.leaf_count[slot];    // (leaves of more than 30 triangles)
                }
                if (rem > 0) {
                    const float4* rec = p.records + (size_t)slot * 4;
                    V3 a, ab, ac;
                    pq_triangle(rec[0], rec[1], rec[2], s, a, ab, ac);
                    const V3 b = a + ab, c = a + ac;
                    bool pass = true, allin = true;             // steps 3 and 4
#pragma unroll
                    for (int j = 0; j < KT; j++) {
                        if (j >= K || !pass) break;
                        const float ha = sc_height(n[j], q[j], a), hb = sc_height(n[j], q[j], b), hc = sc_height(n[j], q[j], c);
                        const int above = (ha >= 0.0f) + (hb >= 0.0f) + (hc >= 0.0f), below = (ha < 0.0f) + (hb < 0.0f) + (hc < 0.0f);
                        pass = above + below == 3 && below != 3;     // all three classified (a NaN height is neither), not all BELOW
                        allin = allin && above == 3;
                    }
                    // step 5 only for a triangle that straddles a face
                    if (pass && (allin || rg_clip(p.records, in, slot, R, K)) && pair(k, slot, allin)) done = true;
                }
                rem--;
                cur = rem > 0 ? cur + 1 : kNeedPop;
                rem = rem > 0 ? rem : -1;
            }
            if (cur == kNeedPop) cur = stack.pop();
        } while (cur != kSentinel && !done);
        if (done) break;
    }
    return pops;
}

// Waves per SIMD asked of the compiler for a plane capacity: the planes take 6*KT registers on top of the sections' 40
constexpr int rg_waves(int KT) { return KT <= 2 ? 8 : KT <= 4 ? 6 : KT <= 6 ? 5 : 4; }

// ANY = false: the pairs of each region and how many of them are wholly inside (rt_count_in_regions, and rt_region_offsets' first
// step into the workspace).  ANY = true (any wanted, count and inside not): the traversal ends at the first pair, across instances too.
template <int KT, bool ANY>
__global__ __launch_bounds__(kTriBlock, rg_waves(KT)) void region_count_kernel(const RegParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const float* R = p.regions + (size_t)i * (size_t)(6 * p.planes);
    int32_t total = 0, inside = 0;
    const int32_t pops = rg_trace<KT>(p, stack, R, [&](int32_t) { return true; }, [&](int32_t, int32_t, bool in) {
        total++;
        inside += in ? 1 : 0;
        return ANY;
    });
    if (p.count) p.count[i] = total;
    if (p.inside) p.inside[i] = inside;
    if (p.any) p.any[i] = total > 0 ? 1 : 0;
    if (p.pops) p.pops[i] = pops;
}

// A room's entry while the heap is at work: the key (instance, triangle) as one number, the pair's inside flag, which travels with
// the key in the entry's own inside slot when that field is wanted, and the pair's record slot, which travels in the entry's normal
// (its first word) when normal is wanted, as section_list_kernel carries it.
struct RgItem { uint64_t key; int32_t slot; uint8_t flag; };
struct RgRoom {
    const RegParams& p;
    __device__ __forceinline__ RgItem get(size_t q) const
    {
        RgItem it;
        it.key = pair_key(p.instance[q], p.triangle[q]);
        it.slot = p.normal ? __float_as_int(p.normal[3 * q]) : 0;
        it.flag = p.flag ? p.flag[q] : 0;
        return it;
    }
    __device__ __forceinline__ void put(size_t q, RgItem it) const
    {
        p.instance[q] = (int32_t)(it.key >> 32);
        p.triangle[q] = (int32_t)(uint32_t)it.key;
        if (p.normal) p.normal[3 * q] = __int_as_float(it.slot);
        if (p.flag) p.flag[q] = it.flag;
    }
};

// box_list_kernel's room heap on (instance, triangle) and its early end for fixed rooms without count.  A pair's inside
// flag depends on the region, the instance and the record alone and travels with its key; normal is written after the sort from the
// slot that travelled with it: the rooms are the same bits with and without count and whatever the tree.
template <int KT>
__global__ __launch_bounds__(kTriBlock, rg_waves(KT)) void region_list_kernel(const RegParams p)
{
    extern __shared__ int lds_stack[];                          // [lds_rows(stack_depth)][kTriBlock]
    const int32_t i = (int32_t)blockIdx.x * kTriBlock + (int32_t)threadIdx.x;       // (< n <= INT32_MAX: no overflow)
    if (i >= p.n) return;
    int spill[kMaxStack - kLdsStack];
    TriStack stack = query_stack(lds_stack, spill, p.stack_depth);
    const float* R = p.regions + (size_t)i * (size_t)(6 * p.planes);
    const bool early = !p.offsets && !p.count;
    int32_t total = 0;
    uint64_t filled = 0;                                        // (<= room)
    const int32_t pops = rg_trace<KT>(p, stack, R, [&](int32_t k) {
        if (!early || filled < (uint64_t)p.max_hits) return true;                   // (fixed rooms: start i*M, room M)
        return k <= p.instance[(size_t)i * (size_t)p.max_hits];                     // (the root: the room's greatest key)
    }, [&](int32_t k, int32_t slot, bool in) {
        total++;
        size_t start;
        uint64_t room;
        xl_room(p, i, start, room);                             // (read again per pair: not held across the traversal)
        if (room == 0) return false;
        room_insert(RgRoom{p}, start, room, filled, RgItem{pair_key(k, p.tri_id[slot]), slot, (uint8_t)(in ? 1 : 0)});
        return false;
    });
    size_t start;
    uint64_t room;
    xl_room(p, i, start, room);
    room_sort(RgRoom{p}, start, filled);
    if (p.normal) {
        for (uint64_t j = 0; j < filled; j++) {                 // the sorted entries: normal from the slot
            const size_t q = start + (size_t)j;
            const V3 nn = pq_normal(p, p.instances[p.instance[q]], RgRoom{p}.get(q).slot);
            p.normal[3 * q] = nn.x; p.normal[3 * q + 1] = nn.y; p.normal[3 * q + 2] = nn.z;
        }
    }
    for (uint64_t j = filled; j < room; j++) {                  // padding
        const size_t q = start + (size_t)j;
        p.instance[q] = -1;
        p.triangle[q] = -1;
        if (p.flag) p.flag[q] = 0;
        if (p.normal) { p.normal[3 * q] = 0.0f; p.normal[3 * q + 1] = 0.0f; p.normal[3 * q + 2] = 0.0f; }
    }
    if (p.count) p.count[i] = total;
    if (p.pops) p.pops[i] = pops;
}

}  // namespace

// =====================================================================================
//                                  host side of the C-ABI
// =====================================================================================

struct RtTimer { hipEvent_t start, stop; };

// A caller's ray table (rt_ray_table_create): camera-space directions in the tiled layout of RenderParams::dir_table, whole tiles.
// Immutable once created; owned by the caller, not by a scene.
struct RtRayTable {
    float* d_table;
    int32_t width, height, tiles_x, tiles_y;
    size_t bytes;
};

#define RT_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

namespace {

DevInstance make_dev_instance(const RtInstanceDesc& d, const RtScene& s)
{
    DevInstance o;
    memset(&o, 0, sizeof o);
    o.q_rot = euler2quat(v3(d.rotation[0], d.rotation[1], d.rotation[2]));
    o.q_pose = euler2quat(v3(d.pose[3], d.pose[4], d.pose[5]));
    o.q_inv_pose = euler2quat(v3(d.inv_pose[3], d.inv_pose[4], d.inv_pose[5]));
    o.q_inv_rot = euler2quat(v3(d.inv_rotation[0], d.inv_rotation[1], d.inv_rotation[2]));
    for (int k = 0; k < 3; k++) {
        o.pose_xyz[k] = d.pose[k]; o.inv_pose_xyz[k] = d.inv_pose[k];
        o.scale[k] = d.scale[k]; o.inv_scale[k] = d.inv_scale[k];
    }
    o.identity_inv = 1;
    for (int k = 0; k < 3; k++) if (!(d.scale[k] == 1.0f && d.inv_pose[k] == 0.0f)) o.identity_inv = 0;
    if (!(o.q_inv_pose.x == 1.0f && o.q_inv_pose.y == 0.0f && o.q_inv_pose.z == 0.0f && o.q_inv_pose.w == 0.0f)) o.identity_inv = 0;
    o.unit_inv = (d.scale[0] == 1.0f && d.scale[1] == 1.0f && d.scale[2] == 1.0f &&
                  o.q_inv_pose.x == 1.0f && o.q_inv_pose.y == 0.0f && o.q_inv_pose.z == 0.0f && o.q_inv_pose.w == 0.0f) ? 1 : 0;
    o.root_ref = s.mesh_root_ref[d.mesh_index];
    o.exact_uv = s.mesh_exact_uv[d.mesh_index];
    o.material_index = d.material_index;
    o.mesh_index = d.mesh_index;
    return o;
}

bool instance_ok(const RtInstanceDesc& d, const RtScene& s)
{
    return d.mesh_index >= 0 && d.mesh_index < (int)s.mesh_root_ref.size() &&
           d.material_index >= 0 && d.material_index < s.num_materials;
}

template <class T>
int upload(T** dptr, const std::vector<T>& h, size_t& total)
{
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    RT_HIP(hipMalloc((void**)dptr, bytes));
    if (!h.empty()) RT_HIP(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    total += bytes;
    return 0;
}

int32_t leaf_ref(int64_t slot, int count) { return kLeafFlag | ((count <= 30 ? count : 31) << kSlotBits) | (int32_t)slot; }

bool camera_ok(const RtCameraParams* cam) { return cam && cam->width > 0 && cam->height > 0; }

// the camera of one frame (Camera.cu:23-36: the by-value arguments of render<<<>>>)
void fill_frame(FrameParams& f, const RtCameraParams* cam)
{
    memcpy(f.kinv, cam->K_inv, sizeof f.kinv);
    memcpy(f.D, cam->D, sizeof f.D);
    f.origin[0] = cam->camera_pose[0]; f.origin[1] = cam->camera_pose[1]; f.origin[2] = cam->camera_pose[2];
    f.q_cam = euler2quat(v3(cam->inv_camera_pose[3], cam->inv_camera_pose[4], cam->inv_camera_pose[5]));
}

// the scene's part of the launch parameters
void fill_scene(RenderParams& p, const RtScene* s)
{
    p.records = s->d_records; p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
    p.leaf_count = s->d_leaf_count; p.mesh_flags = s->d_mesh_flags;
    p.instances = s->d_instances; p.materials = s->d_materials;
    p.num_instances = (int32_t)s->instances.size();
    p.stack_depth = s->max_stack;
}

// count cameras (same width/height) -> the per-frame part of the launch parameters
// (no_images: rt_render_gbuffer without colour frames -- d_imgs is null, every frame's img stays null and the pitch is not looked at)
int fill_params(RenderParams& p, const RtScene* s, const RtCameraParams* cams, uint8_t* const* d_imgs, int count, size_t pitch, bool no_images = false)
{
    if (!s || !cams || (!d_imgs != no_images) || count < 1 || count > kMaxBatch || !camera_ok(&cams[0]) || (!no_images && pitch < (size_t)cams[0].width * 3)) return RT_E_INVALID;
    memset(&p, 0, sizeof p);
    p.width = cams[0].width; p.height = cams[0].height;
    p.num_frames = count;
    for (int i = 0; i < count; i++) {
        const RtCameraParams* cam = &cams[i];
        if (cam->width != p.width || cam->height != p.height || (!no_images && !d_imgs[i])) return RT_E_INVALID;
        FrameParams& f = p.frames[i];
        fill_frame(f, cam);
        f.img = no_images ? nullptr : d_imgs[i];
        f.rank = 0; f.local_rows = p.height;
    }
    fill_scene(p, s);
    p.pitch = pitch;
    p.local_rows = p.height; p.stripe_rows = p.height; p.rank = 0; p.num_ranks = 1;
    return RT_OK;
}

// RT_TRACE_FILE diagnostics: a zeroed [waves][16] u64 buffer for the kernel's stamps, written to the file afterwards
hipError_t trace_begin(RenderParams& p, size_t n)
{
    hipError_t e = hipMalloc((void**)&p.trace, n * 8);
    return e != hipSuccess ? e : hipMemset(p.trace, 0, n * 8);
}
hipError_t trace_end(RenderParams& p, size_t n, const char* path, hipStream_t stream)
{
    std::vector<unsigned long long> h(n);
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipMemcpy(h.data(), p.trace, n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(p.trace);
    p.trace = nullptr;
    if (e == hipSuccess)
        if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), 8, n, f); fclose(f); }
    return e;
}

// Launch with heavy-first tile order.  The order a launch reads was sorted from the costs of an earlier
// frame by tile_sort_kernel on the scene's own side stream, so sorting never sits between two frames on the caller's
// stream; the host switches to a new order when it finds its sort finished (an event query, no wait) and keeps at most one
// sort in flight per frame size: a sort writes the buffer no queued or running launch reads (every launch issued before the
// sort used the other buffer or has finished -- the sort waits for the last ordered launch of every stream that renders this
// size, up to four at a time; a stream slot whose launch has finished is handed to the next new stream -- and every launch
// issued while the sort is pending still reads the other buffer).  Nothing here waits on the host or synchronises the
// device, except when a FIFTH frame size evicts an idle state (its arrays are freed); a launch that finds no state it
// may use renders in natural order.
namespace {
// whether every ordered launch issued on the entry's stream has finished.  Launches since the stream's last recorded event (dirty):
// an idle stream has finished them all; on a busy one the event is recorded now, behind them, and tells a later call.
bool seen_finished(RtScene::TileOrder::Seen& e)
{
    if (e.dirty) {
        const hipError_t q = hipStreamQuery(e.stream);
        if (q == hipSuccess) { e.dirty = e.recorded = false; return true; }
        (void)hipGetLastError();
        if (q != hipErrorNotReady) { e.dirty = e.recorded = false; return true; }   // (a stream the application has destroyed: its work is over)
        e.dirty = false;
        if (hipEventRecord(e.done, e.stream) != hipSuccess) { (void)hipGetLastError(); return true; }
        e.recorded = true;
        return false;
    }
    if (!e.recorded) return true;                               // (never launched, or everything it launched was seen finished)
    const bool done = hipEventQuery(e.done) == hipSuccess;
    if (!done) (void)hipGetLastError();
    return done;
}

bool order_state_idle(RtScene::TileOrder& o)
{
    if (o.pending) { if (hipEventQuery(o.sort_done) != hipSuccess) return false; o.cur = o.target; o.pending = false; }
    for (auto& e : o.seen) if (e.used && !seen_finished(e)) return false;
    return true;
}
}  // namespace

// a tree of L levels never holds more than L - 1 postponed nodes (see StackT): the kernels without the private overflow.
// RT_STACK_SPILL=1 forces the general kernels (read once per process: tests/test_gpu_parity.py runs a parity scene in a child
// process with it; test_stack_depth_at_the_lds_boundary renders chains of 15..20 levels through whichever form their depth selects)
bool lds_stack_suffices(const RenderParams& p)
{
    static const bool forced = [] { const char* e = getenv("RT_STACK_SPILL"); return e && e[0] == '1'; }();
    return !forced && p.stack_depth - 1 <= kLdsStack;
}

// ---- view records (RtScene::ViewPool; view_records_kernel; render_kernel<.., VIEW>) -------------------------------------------
// RT_VIEW_RECORDS=0: never (tests run parity scenes both ways).  RT_VIEW_MIN_RAYS=k: a launch qualifies when a frame brings at
// least k rays per view record it costs to write (default 8: a record is written once and read by tens of rays; below that --
// a rank's thin stripes of a frame, a huge tree under a small frame -- the pre-pass would cost more than the subtractions).
// RT_VIEW_MIN_FRAMES=f: ... and when it carries at least f frames (default 4): the pre-pass is a launch of its own in front of
// the render kernel, a few microseconds that a batch shares and a single frame pays alone (measured on c2: 32 frames per
// launch -3 % / -6 % for the mid / near camera, one frame per launch +4 % / +7 %; profiles/r05_experiments/view_records_asm_ab.log).
constexpr size_t kViewMaxBytes = (size_t)3 << 30;            // records + pool stay below 4 GiB: offsets are 32 bits

int view_mode()
{
    static const int mode = [] { const char* e = getenv("RT_VIEW_RECORDS"); return e && e[0] == '0' ? 0 : 1; }();
    return mode;
}

// RT_VIEW_MAX_BYTES: what the pool of ONE scene may take (default 1 GiB; never more than keeps records + pool below 4 GiB)
size_t view_budget()
{
    static const size_t b = [] {
        const char* e = getenv("RT_VIEW_MAX_BYTES");
        size_t v = e && *e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 30;
        return v > kViewMaxBytes ? kViewMaxBytes : v;
    }();
    return b;
}

// static eligibility of the scene (decided once; the caller holds call_mu)
void view_decide(RtScene* s)
{
    RtScene::ViewPool& v = s->view;
    if (v.decided) return;
    v.decided = true;
    int32_t cap = 0;
    for (const auto& rf : s->mesh_refit) cap = std::max(cap, rf.int_cap);
    // (an instance may be given another mesh later, rt_scene_update_instance: every instance gets room for the largest)
    // ... behind the frame's ray headers, one 64-byte block per instance (view_records_kernel): they count as records of the view,
    // so every size derived from frame_records (view_resize, rt_scene_reserve_views, rt_scene_memory) carries them
    const int32_t headers = (int32_t)s->instances.size();
    v.frame_records = headers + cap * (int32_t)s->instances.size();
    v.inst_first.resize(s->instances.size());
    for (size_t i = 0; i < s->instances.size(); i++) v.inst_first[i] = headers + (int32_t)i * cap;
    v.usable = cap > 0 && s->records_bytes > 0 && !s->instances.empty() && s->instances.size() <= (size_t)kMaxViewInstances &&
               s->records_bytes + (size_t)v.frame_records * 64 <= kViewMaxBytes;
}

// The record array moves into a new allocation with a pool of `slots` x `frames` views as its tail (slots: three, or as many as the
// budget allows).  The caller holds call_mu -- no other launch of this scene can be prepared meanwhile -- and the device is drained
// first: nothing reads the old block afterwards, so it is freed here.  RT_OK, RT_E_NOMEM (budget or allocation), or a HIP error.
int view_resize(RtScene* s, int frames)
{
    RtScene::ViewPool& v = s->view;
    const size_t frame_bytes = (size_t)v.frame_records * 64, base = (s->records_bytes + 255) & ~(size_t)255;
    const size_t room = std::min(view_budget(), kViewMaxBytes > base ? kViewMaxBytes - base : 0);
    int slots = 3;
    while (slots > 1 && frame_bytes * (size_t)slots * (size_t)frames > room) slots--;
    if (frames < 1 || frame_bytes * (size_t)slots * (size_t)frames > room) return RT_E_NOMEM;
    const size_t total = base + frame_bytes * (size_t)slots * (size_t)frames;
    float4* block = nullptr;
    RT_HIP(hipDeviceSynchronize());
    if (hipMalloc((void**)&block, total) != hipSuccess) { (void)hipGetLastError(); return RT_E_NOMEM; }
    hipError_t e = hipMemcpy(block, s->d_records, s->records_bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { (void)hipFree(block); return (int)e; }
    (void)hipFree(s->d_records);
    s->device_bytes += total;
    s->device_bytes -= std::min(s->device_bytes, s->records_alloc_bytes);
    s->d_records = block;
    s->records_alloc_bytes = total;
    v.base_bytes = base; v.slot_frames = frames; v.slots = slots; v.grows++;
    for (auto& sl : v.slot) { sl.used = false; sl.stream = nullptr; }
    v.written = RtScene::ViewPool::Written();                   // (the views of the last launch did not move with the records)
    return RT_OK;
}

// RT_DIR_TABLE=0: no launch reads camera-space directions from a table (read once; the A/B switch, and the tests')
int dir_table_mode()
{
    static const int mode = [] { const char* e = getenv("RT_DIR_TABLE"); return e && e[0] == '0' ? 0 : 1; }();
    return mode;
}

// RT_VIEW_CULL=0: the pre-pass writes every view with the boxes as they are (read once; the A/B switch, and the tests')
int view_cull_mode()
{
    static const int mode = [] { const char* e = getenv("RT_VIEW_CULL"); return e && e[0] == '0' ? 0 : 1; }();
    return mode;
}

// The direction table of a launch that got view slot `sl` (RenderParams::dir_table): for a primary launch of one rank and at least two
// frames -- never the ordered grid, then -- whose frames all carry the first frame's K_inv and D bit for bit.  Returns the slot's buffer,
// grown first if this image needs more room, or null: the launch then renders as it did without tables.
float* dir_table_prepare(RtScene* s, RtScene::ViewPool::Slot& sl, const RenderParams& p)
{
    RtScene::ViewPool& v = s->view;
    const size_t ntiles = (size_t)p.tiles_x * (size_t)p.tiles_y;
    if (!dir_table_mode() || p.num_ranks != 1 || p.num_frames < 2 || ntiles < 1 || ntiles > ((size_t)1 << 24)) return nullptr;
    static_assert(offsetof(FrameParams, kinv) == 0 && offsetof(FrameParams, D) == sizeof(float) * 9, "K_inv and D lead the frame's parameters");
    for (int k = 1; k < p.num_frames; k++)
        if (memcmp(&p.frames[k], &p.frames[0], sizeof(float) * 13) != 0) return nullptr;
    const size_t need = ntiles * 3 * 64 * sizeof(float);
    if (sl.dirs_bytes < need) {
        // whatever last read the old buffer was queued before the slot's event was recorded (a slot that was never used has neither)
        if (sl.d_dirs && sl.done && hipEventSynchronize(sl.done) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        float* block = nullptr;
        if (hipMalloc((void**)&block, need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        (void)hipFree(sl.d_dirs);
        // (not in s->device_bytes: rt_scene_info / rt_scene_memory promise records + pool + the scene's arrays, and applications size
        // their budgets by that sum; the tables have a count of their own, rt_scene_dir_table_stats)
        std::lock_guard<std::mutex> lock(v.m);
        v.dir_bytes += need; v.dir_bytes -= sl.dirs_bytes;
        if (sl.d_dirs) v.dir_grows++;                           // (a slot's first buffer is not a growth)
        sl.d_dirs = block; sl.dirs_bytes = need;
    }
    return sl.d_dirs;
}

// Decides whether this launch renders through view records; if so: a slot of the pool (grown when needed and allowed), the launch's
// view parameters in `p`, the pre-pass queued on `stream`.  Returns the slot (view_done records its event after the render kernel) or
// -1: the launch then runs the kernels without views -- same pixels.  The caller holds call_mu from here to view_done.
// `samples`: primary rays per pixel (the samples-only extension kernel: its jittered rays share the frame's origin too).
// `primary`: the caller is launch() with p.tiles_x / tiles_y set -- the launch may also get a direction table (dir_table_prepare).
// `caller_table` (rt_render_gbuffer_table): the launch reads this table, not one of the library's -- the pre-pass writes none and the
// launch counts in neither dir_launches nor dir_skipped, which keep describing the library's own tables.
int view_prepare(RtScene* s, RenderParams& p, hipStream_t stream, int samples = 1, bool primary = false, const float* caller_table = nullptr)
{
    if (!view_mode() || !s || p.num_instances < 1 || p.num_instances > kMaxViewInstances || p.num_ranks < 1) return -1;
    RtScene::ViewPool& v = s->view;
    view_decide(s);
    if (!v.usable || (size_t)p.num_instances != s->instances.size()) return -1;
    ViewJob job;
    job.n = p.num_instances; job.total = 0;
    for (int i = 0; i < job.n; i++) {
        const RtScene::MeshRefit& rf = s->mesh_refit[(size_t)s->instances[(size_t)i].mesh_index];
        job.first[i] = v.inst_first[(size_t)i]; job.node_base[i] = rf.node_base; job.count[i] = rf.int_cap;
        job.total += rf.int_cap;
    }
    static const long min_rays = [] { const char* e = getenv("RT_VIEW_MIN_RAYS"); long k = e ? atol(e) : 8; return k < 0 ? 0 : k; }();
    static const int min_frames = [] { const char* e = getenv("RT_VIEW_MIN_FRAMES"); int k = e ? atoi(e) : 4; return k < 1 ? 1 : k; }();
    if (job.total <= 0 || (long long)p.num_frames * samples < min_frames || (long long)job.total * min_rays > (long long)p.width * p.local_rows * samples) {
        if (getenv("RT_VIEW_DEBUG")) fprintf(stderr, "rt view: not for this launch (records %d, frames %d of %d, rays per frame %lld, rays per record wanted %ld)\n",
                                             job.total, p.num_frames, min_frames, (long long)p.width * p.local_rows, min_rays);
        return -1;
    }
    auto count = [&](uint64_t RtScene::ViewPool::*field) { std::lock_guard<std::mutex> lock(v.m); (v.*field)++; };
    count(&RtScene::ViewPool::launches);
    const size_t frame_bytes = (size_t)v.frame_records * 64;
    if (p.num_frames > v.slot_frames) {
        // the pool is too small for this launch.  Reserved by the application: it stays as it is.  Else it grows to the next of
        // 1 / 4 / 8 / 16 / 32 frames per slot -- or to exactly this launch's frames where the budget allows no more -- in a call
        // that blocks until the device is idle (at most five times in a scene's life; see rt_render_batch in rt_hip.h)
        if (v.reserved) { count(&RtScene::ViewPool::fallbacks); return -1; }
        int want = 1;
        while (want < p.num_frames) want = want == 1 ? 4 : want * 2;
        want = std::min(want, (int)kMaxBatch);
        int rc = view_resize(s, want);
        if (rc == RT_E_NOMEM && want != p.num_frames) rc = view_resize(s, p.num_frames);
        if (rc != RT_OK) {
            if (rc != RT_E_NOMEM) v.usable = false;             // (a HIP error: this scene renders without views from now on)
            count(&RtScene::ViewPool::fallbacks);
            return -1;
        }
    }
    int use = -1;
    for (int k = 0; k < v.slots && use < 0; k++) if (v.slot[k].used && v.slot[k].stream == stream) use = k;   // stream order protects it
    for (int k = 0; k < v.slots && use < 0; k++) if (!v.slot[k].used) use = k;
    for (int k = 0; k < v.slots && use < 0; k++) {                                                            // its last launch has finished
        if (hipEventQuery(v.slot[k].done) == hipSuccess) use = k;
        else (void)hipGetLastError();
    }
    if (use < 0) { count(&RtScene::ViewPool::fallbacks); return -1; }                                        // (all busy on other streams)
    if (!v.slot[use].done && hipEventCreateWithFlags(&v.slot[use].done, hipEventDisableTiming) != hipSuccess) { count(&RtScene::ViewPool::fallbacks); return -1; }
    v.slot[use].used = true; v.slot[use].stream = stream;
    p.records = s->d_records;                                   // (fill_params read it before a possible move)
    p.view_base = (uint32_t)(v.base_bytes + (size_t)use * v.slot_frames * frame_bytes);
    p.view_frame_stride = (uint32_t)frame_bytes;
    for (int i = 0; i < job.n; i++) p.view_inst_off[i] = (int32_t)(((int64_t)job.first[i] - job.node_base[i]) * 64);
    job.record_blocks = (uint32_t)(((size_t)job.total * 4 + (size_t)job.n + 255) / 256);
    p.dir_table = caller_table ? caller_table : (primary && samples == 1) ? dir_table_prepare(s, v.slot[use], p) : nullptr;
    // (four tiles per workgroup, the workgroups dealt to the rows of the grid)
    const size_t rows = ((size_t)p.num_frames + kViewFrameChunk - 1) / kViewFrameChunk;
    job.dir_blocks = p.dir_table && !caller_table ? (uint32_t)((((size_t)p.tiles_x * (size_t)p.tiles_y + 3) / 4 + rows - 1) / rows) : 0u;
    // culled views go to the kernels that report no visit counts: the primary and G-buffer launches.  The samples-only extension
    // kernel counts node pops against the oracle's and reads the boxes as they are.
    job.cull = primary && view_cull_mode() ? 1 : 0;
    job.records_end = (uint32_t)(s->records_bytes / 64);
    hipLaunchKernelGGL(view_records_kernel, dim3(job.record_blocks + job.dir_blocks, (unsigned)rows), dim3(256), 0, stream, p, job);
    if (hipGetLastError() != hipSuccess) { p.dir_table = nullptr; count(&RtScene::ViewPool::fallbacks); return -1; }
    {
        // (what rt_scene_view_cull_stats counts: the views this launch wrote, while they stand)
        RtScene::ViewPool::Written& w = v.written;
        w.culled = job.cull != 0; w.view_base = p.view_base; w.frames = p.num_frames; w.n = job.n;
        for (int i = 0; i < job.n; i++) { w.first[i] = job.first[i]; w.count[i] = job.count[i]; }
    }
    if (!caller_table) count(p.dir_table ? &RtScene::ViewPool::dir_launches : &RtScene::ViewPool::dir_skipped);
    return use;
}

void view_done(RtScene* s, int slot, hipStream_t stream)
{
    if (slot < 0) return;
    (void)hipEventRecord(s->view.slot[slot].done, stream);     // (still under the call_mu view_prepare was called under)
}

int launch_ordered(RtScene* s, RenderParams& p, hipStream_t stream, int synchronize, bool view)
{
    RtScene::TileOrderCache& cache = s->order;
    std::lock_guard<std::mutex> lock(cache.m);
    const int ntiles = p.tiles_x * p.tiles_y;
    // (a high-priority side stream was tried: frames alternating between two streams went from 0.111 to 0.126 ms with it)
    if (!cache.sort_stream) RT_HIP(hipStreamCreateWithFlags(&cache.sort_stream, hipStreamNonBlocking));
    RtScene::TileOrder* o = nullptr;
    for (auto& e : cache.entry) if (e.ntiles && e.tiles_x == p.tiles_x && e.tiles_y == p.tiles_y) o = &e;
    if (!o) {                                                   // a size not seen before: a free state, else the least recently used idle one
        for (auto& e : cache.entry) if (!e.ntiles && !o) o = &e;
        if (!o) {
            RtScene::TileOrder* lru = nullptr;
            for (auto& e : cache.entry) if (!lru || e.last_used < lru->last_used) lru = &e;
            if (order_state_idle(*lru)) {
                (void)hipFree(lru->d_cost);
                lru->d_cost = lru->d_keys = lru->d_order[0] = lru->d_order[1] = nullptr;
                lru->tiles_x = lru->tiles_y = lru->ntiles = 0; lru->cur = -1; lru->pending = false; lru->launches = lru->sorted_at = 0;
                for (auto& e : lru->seen) e.used = e.dirty = e.recorded = false;
                o = lru;
            }
        }
        if (o) {
            if (!o->sort_done) {
                RT_HIP(hipEventCreateWithFlags(&o->sort_done, hipEventDisableTiming));
                for (auto& e : o->seen) RT_HIP(hipEventCreateWithFlags(&e.done, hipEventDisableTiming));
            }
            RT_HIP(hipMalloc((void**)&o->d_cost, (size_t)ntiles * 4 * sizeof(int32_t)));
            RT_HIP(hipMemsetAsync(o->d_cost, 0, (size_t)ntiles * sizeof(int32_t), stream));
            o->d_keys = o->d_cost + ntiles; o->d_order[0] = o->d_keys + ntiles; o->d_order[1] = o->d_order[0] + ntiles;
            o->tiles_x = p.tiles_x; o->tiles_y = p.tiles_y; o->ntiles = ntiles;
        }
    }
    RtScene::TileOrder::Seen* mine = nullptr;
    if (o) {
        o->last_used = ++cache.tick;
        if (o->pending && hipEventQuery(o->sort_done) == hipSuccess) { o->cur = o->target; o->pending = false; }
        for (auto& e : o->seen) if (e.used && e.stream == stream) mine = &e;
        if (!mine) for (auto& e : o->seen) if (!e.used) { mine = &e; break; }
        if (!mine) {                                            // all four slots taken: the one whose launches finished longest ago
            for (auto& e : o->seen)
                if (seen_finished(e) && (!mine || e.tick < mine->tick)) mine = &e;
        }
        if (mine) { mine->used = true; mine->stream = stream; mine->tick = cache.tick; }
    }
    p.tile_order = (mine && o->cur >= 0) ? o->d_order[o->cur] : nullptr;
    p.tile_cost = mine ? o->d_cost : nullptr;
    // A new order is sorted every RT_TILE_SORT_INTERVAL-th launch (default 4), on the side stream, from the costs the launches so far
    // have left.  It must not start before every launch that may still read the buffer it writes has finished -- every ordered launch
    // issued BEFORE this one, on any stream (this one reads d_order[cur], the sort writes the other buffer) -- so it runs WHILE this
    // frame renders: a device-wide synchronise after the frame (the reference's loop synchronises every two frames) finds it done.
    // Round 6: the events that tell it are recorded WHEN A SORT IS ISSUED, on every stream that has launched since its last one --
    // not after every launch as before: a recorded event is a marker packet between two kernels of the stream, and back-to-back
    // launches with a marker in between start 7 us apart where launches without start 0 us apart
    // (profiles/r06_experiments/single_frame_gap.md: rocprofv3 kernel-trace timestamps of 60 back-to-back launches, three settings).
    // (This launch rewrites the cost array while the sort reads it: a tile's key is computed once and kept, and whatever the
    // values, the result is a permutation.)
    static const int interval = [] { const char* e = getenv("RT_TILE_SORT_INTERVAL"); int v = e ? atoi(e) : 4; return v < 1 ? 1 : v; }();
    if (mine && !o->pending && o->launches >= 1 && (o->cur < 0 || o->launches + 1 - o->sorted_at >= (uint64_t)interval)) {
        for (auto& e : o->seen) {
            if (!e.used || !e.dirty) continue;
            e.dirty = false;
            if (hipEventRecord(e.done, e.stream) != hipSuccess) {           // (a stream the application has destroyed since: its work is over)
                (void)hipGetLastError();
                if (&e != mine) e.used = false;
                e.recorded = false;
                continue;
            }
            e.recorded = true;
        }
        // ... and the sort is QUEUED before the frame (after a synchronise it finds an empty chip); its workgroup is four waves, which
        // find room on a saturated chip too (see tile_sort_kernel)
        o->sorted_at = o->launches + 1;
        o->target = o->cur < 0 ? 0 : o->cur ^ 1;
        for (auto& e : o->seen) if (e.used && e.recorded) RT_HIP(hipStreamWaitEvent(cache.sort_stream, e.done, 0));
        hipLaunchKernelGGL(tile_sort_kernel, dim3(1), dim3(kSortThreads), 0, cache.sort_stream, o->d_cost, ntiles, o->d_keys, o->d_order[o->target]);
        RT_HIP(hipGetLastError());
        RT_HIP(hipEventRecord(o->sort_done, cache.sort_stream));
        o->pending = true;
    }
    const size_t lds = (size_t)(lds_stack_suffices(p) ? lds_block_rows<false, false, false>(p.stack_depth) : lds_block_rows<false, false, true>(p.stack_depth)) *
                       kPrimBlock * sizeof(int) + 2 * sizeof(int);
    const dim3 grid((unsigned)ntiles * (unsigned)p.num_frames);
    if (lds_stack_suffices(p)) {
        if (view) hipLaunchKernelGGL((render_kernel<false, false, true, false, true>), grid, dim3(kPrimBlock), lds, stream, p);
        else hipLaunchKernelGGL((render_kernel<false, false, true, false>), grid, dim3(kPrimBlock), lds, stream, p);
    } else {
        if (view) hipLaunchKernelGGL((render_kernel<false, false, true, true, true>), grid, dim3(kPrimBlock), lds, stream, p);
        else hipLaunchKernelGGL((render_kernel<false, false, true>), grid, dim3(kPrimBlock), lds, stream, p);
    }
    RT_HIP(hipGetLastError());
    if (o) o->launches++;
    if (mine) mine->dirty = true;
    if (synchronize) RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

int launch(RenderParams& p, bool debug, hipStream_t stream, int synchronize, RtScene* scene = nullptr, bool stats = false)
{
    if (p.width <= 0 || p.local_rows < 0) return RT_E_INVALID;
    if (p.local_rows == 0) return RT_OK;
    p.tiles_x = (p.width + kPrimTile - 1) / kPrimTile;
    p.tiles_y = (p.local_rows + kPrimTile - 1) / kPrimTile;
    // (one size for whichever kernel is launched below: the spare row of the optimistic stack costs the instrumented kernels nothing)
    const size_t lds = (size_t)(lds_stack_suffices(p) ? lds_rows(p.stack_depth) : lds_block_rows<false, false, true>(p.stack_depth)) * kPrimBlock * sizeof(int);
    // tile (x, y) of frame z: the kernel takes its tile's coordinates from the workgroup's
    const size_t ntiles = (size_t)p.tiles_x * p.tiles_y, nframes = (size_t)p.num_frames;
    dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)p.num_frames), block(kPrimBlock);
    const char* trace_file = getenv("RT_TRACE_FILE");                               // diagnostics only
    // Heavy-first dispatch (RT_TILE_ORDER=0 turns it off): for one frame per launch with enough tiles to have a tail worth
    // hiding.  Batches do not use it: the tail of one frame already overlaps the bulk of the next, and measured with the
    // order applied across all frames of a batch (workgroup b -> frame b % F of the tile with rank b / F) whole-frame batches ran -2 % (far) to +4 %
    // (near), a rank's stripes of 32 frames -6 % on one stream but no better than the two alternating streams bench.py uses.
    // (RT_TRACE_ORDERED=1 with RT_TRACE_FILE: the stamps of the heavy-first launch itself, for tools/trace_one.py)
    const bool trace_ordered = trace_file && getenv("RT_TRACE_ORDERED");
    const int view_slot = (scene && !debug && !trace_file) ? view_prepare(scene, p, stream, 1, true) : -1;
    const bool table = view_slot >= 0 && p.dir_table != nullptr;     // (one rank, two frames or more: not a launch the ordered grid takes)
    struct ViewDone {                                           // (whichever way this function returns after the render kernel was queued)
        RtScene* s; int slot; hipStream_t stream;
        ~ViewDone() { view_done(s, slot, stream); }
    } view_guard{scene, view_slot, stream};
    if (scene && !debug && (!trace_file || trace_ordered) && !p.hit_instance && !p.hit_triangle && ntiles >= 1024 && ntiles * nframes <= ((size_t)1 << 30)) {
        static const bool enabled = [] { const char* e = getenv("RT_TILE_ORDER"); return !(e && e[0] == '0'); }();
        // ... and (round 6) a rank's STRIPES of a few frames: at eight ranks a group of 20 frames is two and a half frames' worth of
        // work per launch and ends, like a single frame, in a tail of a few long waves (RT_TILE_ORDER_STRIPES=0 turns this part off)
        static const bool stripes_too = [] { const char* e = getenv("RT_TILE_ORDER_STRIPES"); return !(e && e[0] == '0'); }();
        const bool thin_stripes = stripes_too && p.num_ranks > 1 && p.num_frames > 1 && ntiles * nframes < (size_t)4 * 32768;
        if (enabled && !stats && ((p.num_frames == 1 && ntiles >= 8192) || thin_stripes)) {   // (8x8-pixel tiles: half a million pixels)
            if (!trace_ordered) return launch_ordered(scene, p, stream, synchronize, view_slot >= 0);
            const size_t n = ntiles * nframes * (kPrimBlock / 64) * 16;
            RT_HIP(trace_begin(p, n));
            const int rc = launch_ordered(scene, p, stream, 1, false);
            const hipError_t e = trace_end(p, n, trace_file, stream);
            return rc ? rc : (int)e;
        }
    }
    if (p.tiles_y > 65535) return RT_E_INVALID;                 // (a grid's y and z end at 65 535: frames of more than 524 280 rows; the ordered grid above is one-dimensional)
    const size_t trace_n = ntiles * nframes * (kPrimBlock / 64) * 16;
    if (trace_file) RT_HIP(trace_begin(p, trace_n));
    if (trace_file && getenv("RT_TRACE_PROF")) hipLaunchKernelGGL((render_kernel<false, true>), grid, block, lds, stream, p);
    else if (debug) hipLaunchKernelGGL((render_kernel<true, false>), grid, block, lds, stream, p);
    else if (stats) {                                           // rt_scene_loop_stats: the same choices as below, the instrumented copies
        if (lds_stack_suffices(p)) {
            if (table) hipLaunchKernelGGL((render_kernel<false, false, false, false, true, true, true>), grid, block, lds, stream, p);
            else if (view_slot >= 0) hipLaunchKernelGGL((render_kernel<false, false, false, false, true, true>), grid, block, lds, stream, p);
            else hipLaunchKernelGGL((render_kernel<false, false, false, false, false, true>), grid, block, lds, stream, p);
        } else {
            if (table) hipLaunchKernelGGL((render_kernel<false, false, false, true, true, true, true>), grid, block, lds, stream, p);
            else if (view_slot >= 0) hipLaunchKernelGGL((render_kernel<false, false, false, true, true, true>), grid, block, lds, stream, p);
            else hipLaunchKernelGGL((render_kernel<false, false, false, true, false, true>), grid, block, lds, stream, p);
        }
    }
    else if (lds_stack_suffices(p)) {
        if (table) hipLaunchKernelGGL((render_kernel<false, false, false, false, true, false, true>), grid, block, lds, stream, p);
        else if (view_slot >= 0) hipLaunchKernelGGL((render_kernel<false, false, false, false, true>), grid, block, lds, stream, p);
        else hipLaunchKernelGGL((render_kernel<false, false, false, false>), grid, block, lds, stream, p);
    } else {
        if (table) hipLaunchKernelGGL((render_kernel<false, false, false, true, true, false, true>), grid, block, lds, stream, p);
        else if (view_slot >= 0) hipLaunchKernelGGL((render_kernel<false, false, false, true, true>), grid, block, lds, stream, p);
        else hipLaunchKernelGGL((render_kernel<false, false>), grid, block, lds, stream, p);
    }
    RT_HIP(hipGetLastError());
    if (trace_file) RT_HIP(trace_end(p, trace_n, trace_file, stream));
    if (synchronize) RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

// rt_render_gbuffer's launch: the un-ordered grid and the batch launch's choices of launch() -- the stack form by the tree's depth; view
// records when view_prepare grants a slot (four frames or more, at most kMaxViewInstances instances, ...), with the direction table
// when the frames share K_inv and D; plain records otherwise -- each as the gbuffer_kernel instantiation of that form.
// `caller_table` (rt_render_gbuffer_table): every form reads it -- view records when a slot is granted, plain records otherwise.
int launch_gbuffer(RtScene* scene, RenderParams& p, const GBufParams& g, hipStream_t stream, const float* caller_table = nullptr)
{
    if (p.width <= 0 || p.local_rows <= 0) return RT_E_INVALID;
    p.tiles_x = (p.width + kPrimTile - 1) / kPrimTile;
    p.tiles_y = (p.local_rows + kPrimTile - 1) / kPrimTile;
    if (p.tiles_y > 65535) return RT_E_INVALID;                 // (a grid's y ends at 65 535, as in launch())
    const bool shallow = lds_stack_suffices(p);
    const size_t lds = (size_t)(shallow ? lds_rows(p.stack_depth) : lds_block_rows<false, false, true>(p.stack_depth)) * kPrimBlock * sizeof(int);
    const dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)p.num_frames), block(kPrimBlock);
    const int view_slot = view_prepare(scene, p, stream, 1, true, caller_table);
    if (caller_table) p.dir_table = caller_table;               // (view_prepare leaves null where it grants no slot)
    const bool table = view_slot >= 0 && p.dir_table != nullptr;
    if (caller_table && view_slot < 0) {
        if (shallow) hipLaunchKernelGGL((gbuffer_kernel<false, false, true>), grid, block, lds, stream, p, g);
        else hipLaunchKernelGGL((gbuffer_kernel<true, false, true>), grid, block, lds, stream, p, g);
    } else if (shallow) {
        if (table) hipLaunchKernelGGL((gbuffer_kernel<false, true, true>), grid, block, lds, stream, p, g);
        else if (view_slot >= 0) hipLaunchKernelGGL((gbuffer_kernel<false, true, false>), grid, block, lds, stream, p, g);
        else hipLaunchKernelGGL((gbuffer_kernel<false, false, false>), grid, block, lds, stream, p, g);
    } else {
        if (table) hipLaunchKernelGGL((gbuffer_kernel<true, true, true>), grid, block, lds, stream, p, g);
        else if (view_slot >= 0) hipLaunchKernelGGL((gbuffer_kernel<true, true, false>), grid, block, lds, stream, p, g);
        else hipLaunchKernelGGL((gbuffer_kernel<true, false, false>), grid, block, lds, stream, p, g);
    }
    const hipError_t e = hipGetLastError();
    view_done(scene, view_slot, stream);
    return e == hipSuccess ? RT_OK : (int)e;
}

// rt_render_gbuffer_rolling's launch: launch_gbuffer's grid, tile limits and stack form, always over plain records and the caller's
// table -- no view_prepare call: the launch takes no view slot, grows no pool and is counted by neither statistic.
int launch_gbuffer_rolling(RenderParams& p, const GBufParams& g, const RollParams& r, hipStream_t stream, const float* caller_table)
{
    if (p.width <= 0 || p.local_rows <= 0 || !caller_table) return RT_E_INVALID;
    p.tiles_x = (p.width + kPrimTile - 1) / kPrimTile;
    p.tiles_y = (p.local_rows + kPrimTile - 1) / kPrimTile;
    if (p.tiles_y > 65535) return RT_E_INVALID;                 // (a grid's y ends at 65 535, as in launch())
    const bool shallow = lds_stack_suffices(p);
    const size_t lds = (size_t)(shallow ? lds_rows(p.stack_depth) : lds_block_rows<false, false, true>(p.stack_depth)) * kPrimBlock * sizeof(int);
    const dim3 grid((unsigned)p.tiles_x, (unsigned)p.tiles_y, (unsigned)p.num_frames), block(kPrimBlock);
    p.dir_table = caller_table;
    if (shallow) hipLaunchKernelGGL((rolling_gbuffer_kernel<false>), grid, block, lds, stream, p, g, r);
    else hipLaunchKernelGGL((rolling_gbuffer_kernel<true>), grid, block, lds, stream, p, g, r);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RT_OK : (int)e;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

// the hash of the kernel sources and build flags this binary was compiled from (cuda-raytracing_amd/_build.py passes it; a
// build by other means says so).  The text is also what _build.library_code_hash() finds in the file without loading it.
#ifndef RT_CODE_HASH
#define RT_CODE_HASH "built-without-it"
#endif
const char* rt_build_info(void)
{
    static const char info[] = "RT_CODE_HASH=" RT_CODE_HASH;
    return info;
}

int rt_device_count(int* count)
{
    if (!count) return RT_E_INVALID;
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e == hipErrorNoDevice) { *count = 0; return RT_OK; }
    return (int)e;
}
int rt_set_device(int device) { RT_HIP(hipSetDevice(device)); return RT_OK; }
int rt_malloc(void** dptr, size_t bytes) { if (!dptr) return RT_E_INVALID; RT_HIP(hipMalloc(dptr, bytes ? bytes : 1)); return RT_OK; }
int rt_malloc_pitch(void** dptr, size_t* pitch, size_t width_bytes, size_t height)
{
    if (!dptr || !pitch) return RT_E_INVALID;
    RT_HIP(hipMallocPitch(dptr, pitch, width_bytes, height));
    return RT_OK;
}
int rt_free(void* dptr) { RT_HIP(hipFree(dptr)); return RT_OK; }
int rt_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream)
{
    RT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    RT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return RT_OK;
}
int rt_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream)
{
    RT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    RT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return RT_OK;
}
int rt_memcpy2d_d2h(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t height, void* stream)
{
    RT_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, hipMemcpyDeviceToHost, (hipStream_t)stream));
    RT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return RT_OK;
}
int rt_stream_synchronize(void* stream) { RT_HIP(hipStreamSynchronize((hipStream_t)stream)); return RT_OK; }
int rt_device_synchronize(void) { RT_HIP(hipDeviceSynchronize()); return RT_OK; }

const char* rt_error_string(int code)
{
    switch (code) {
    case RT_OK: return "ok";
    case RT_E_INVALID: return "rt: invalid argument";
    case RT_E_NOMEM: return "rt: out of host memory";
    case RT_E_DEPTH: return "rt: BVH deeper than the traversal stack";
    case RT_E_NODEVICE: return "rt: no HIP device";
    case RT_E_COMM: return "rt: RCCL unavailable or failed (rt_comm_last_error)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "rt: unknown error";
    }
}

int rt_scene_upload(const RtSceneDesc* desc, RtScene** out)
{
    // tests of the callers' error paths: while RT_TEST_FAIL_UPLOAD=1 is in the environment every upload fails before it touches anything
    if (const char* e = getenv("RT_TEST_FAIL_UPLOAD")) if (e[0] == '1') return RT_E_NOMEM;
    if (!desc || !out || desc->num_meshes < 0 || desc->num_materials < 0 || desc->num_instances < 0) return RT_E_INVALID;
    if ((desc->num_meshes && !desc->meshes) || (desc->num_materials && !desc->materials) ||
        (desc->num_instances && !desc->instances)) return RT_E_INVALID;
    *out = nullptr;
    RtScene* s = new (std::nothrow) RtScene;
    if (!s) return RT_E_NOMEM;
    int rc = RT_OK;
    // One record array and one index space for the whole scene: per mesh its interior nodes, then its triangles in
    // leaf order.  The per-triangle side arrays use the same index (their entries at interior records are unused).
    // The host vectors hold only the parts of meshes that arrive WITH a tree; the part of a mesh the device builds (num_nodes == 0) is
    // a hole of `skipped` records in them: it is never materialised on the host nor copied (the device arrays start from a memset,
    // and the build clears and fills the mesh's part itself) -- for the 260 k-triangle atrium that was 50 MB of zeros written,
    // then copied from pageable memory: a third of the time from file to renderable scene.  A record's index in the device
    // arrays = its index in the vectors + the holes before it; `segments` says which vector ranges go where.
    std::vector<float4> records;
    std::vector<float> tri_uv;
    std::vector<int32_t> tri_id, leaf_count, mesh_flags;
    std::vector<int> build_on_device;               // meshes that arrive without a tree (num_nodes == 0)
    struct Segment { size_t dev_first, vec_first, count; };        // in records
    std::vector<Segment> segments;
    size_t skipped = 0;                             // records of device-built meshes so far
    try {
        for (int mi = 0; mi < desc->num_meshes && rc == RT_OK; mi++) {
            const RtMeshDesc& m = desc->meshes[mi];
            if (m.num_triangles < 0 || (m.num_triangles && (!m.vertices || !m.normals || !m.uvs))) { rc = RT_E_INVALID; break; }
            if (m.num_nodes == 0) {
                // no tree given: the mesh's part of the arrays is reserved here and the tree is built on the device, in place,
                // once the arrays are uploaded (the kernels of rt_scene_rebuild_mesh_device) -- no host tree, no host re-layout
                const int64_t n = m.num_triangles, int_cap = std::max<int64_t>(n - 1, 0);
                const int64_t node_base = (int64_t)(records.size() / 4 + skipped), slot_base = node_base + int_cap;
                if (slot_base + n + 1 > kSlotMask) { rc = RT_E_INVALID; break; }
                skipped += (size_t)(int_cap + n);                // (a hole in the host vectors: see above)
                s->mesh_root_ref.push_back(leaf_ref(slot_base, 0));
                s->mesh_exact_uv.push_back(0);
                RtScene::MeshRefit rf;
                rf.node_base = (int32_t)node_base; rf.int_cap = (int32_t)int_cap; rf.slot_cap = (int32_t)n; rf.levels = 1;
                rf.slot_base = (int32_t)slot_base; rf.num_slots = 0; rf.num_triangles = 0;
                s->mesh_refit.push_back(std::move(rf));
                build_on_device.push_back(mi);
                mesh_flags.push_back(0);                         // (the rebuild on the device sets it)
                continue;
            }
            if (m.num_nodes < 1 || m.num_leaf_indices < 0 || !m.node_bounds || !m.node_children || !m.node_leaf_first || !m.node_leaf_count ||
                (m.num_leaf_indices && !m.leaf_indices)) {
                rc = RT_E_INVALID; break;
            }
            int64_t mesh_interior = 0;
            for (int i = 0; i < m.num_nodes; i++) mesh_interior += m.node_children[2 * i] > 0 ? 1 : 0;
            // (room for any tree over these triangles: rt_scene_rebuild_mesh_device writes a new one in place)
            const int64_t int_cap = std::max<int64_t>(mesh_interior, (int64_t)m.num_triangles - 1);
            const size_t vec_first = records.size() / 4;         // where this mesh's part starts in the host vectors ...
            const int64_t node_base = (int64_t)(vec_first + skipped), slot_base = node_base + int_cap;      // ... and in the device arrays
            if (slot_base + std::max<int64_t>(m.num_leaf_indices, m.num_triangles) + 1 > kSlotMask) { rc = RT_E_INVALID; break; }
            // pass 1: entry of every node (interior -> running interior index, leaf -> slot range), levels
            std::vector<int32_t> entry((size_t)m.num_nodes), level((size_t)m.num_nodes, 0);
            int64_t n_int = 0, n_slot = 0;
            int max_level = 1;
            level[0] = 1;
            for (int i = 0; i < m.num_nodes && rc == RT_OK; i++) {
                const int a = m.node_children[2 * i], b = m.node_children[2 * i + 1];
                if (level[i] == 0) { rc = RT_E_INVALID; break; }          // unreachable or child before parent
                if (a > 0) {                                               // interior test of raycast.cu:66
                    if (a <= i || b <= i || a >= m.num_nodes || b >= m.num_nodes || level[a] || level[b] || a == b) { rc = RT_E_INVALID; break; }
                    level[a] = level[b] = level[i] + 1;
                    max_level = std::max(max_level, level[i] + 1);
                    entry[i] = (int32_t)(node_base + n_int++);
                } else {
                    const int first = m.node_leaf_first[i], count = m.node_leaf_count[i];
                    if (count < 0 || first < 0 || (int64_t)first + count > m.num_leaf_indices) { rc = RT_E_INVALID; break; }
                    entry[i] = leaf_ref(slot_base + n_slot, count);
                    n_slot += count;
                }
            }
            if (rc != RT_OK) break;
            // leaf ranges may overlap in a caller-supplied tree, so the slots actually emitted (the sum of the leaf counts)
            // can exceed num_leaf_indices: the slot field of a ref must still hold them
            if (slot_base + n_slot + 1 > kSlotMask) { rc = RT_E_INVALID; break; }
            if (max_level > kMaxStack) { rc = RT_E_DEPTH; break; }
            s->max_stack = std::max(s->max_stack, max_level);
            // pass 2: emit records
            bool exact_uv = false, unordered = false;
            const int64_t slot_cap = std::max<int64_t>(n_slot, m.num_triangles);
            records.reserve(records.size() + (size_t)(int_cap + slot_cap) * 4 + 4);
            tri_uv.reserve(tri_uv.size() + (size_t)(int_cap + slot_cap) * 6);
            tri_id.reserve(tri_id.size() + (size_t)(int_cap + slot_cap));
            leaf_count.reserve(leaf_count.size() + (size_t)(int_cap + slot_cap));
            records.resize(records.size() + (size_t)int_cap * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            tri_uv.resize(tri_uv.size() + (size_t)int_cap * 6, 0.0f);
            tri_id.resize(tri_id.size() + (size_t)int_cap, -1);
            leaf_count.resize(leaf_count.size() + (size_t)int_cap, 0);
            for (int i = 0; i < m.num_nodes && rc == RT_OK; i++) {
                const int a = m.node_children[2 * i], b = m.node_children[2 * i + 1];
                if (a > 0) {
                    const float* A = m.node_bounds + 6 * (size_t)a;
                    const float* B = m.node_bounds + 6 * (size_t)b;
                    float4* q = &records[((size_t)entry[i] - skipped) * 4];
                    q[0] = make_float4(A[0], A[1], A[2], A[3]);
                    q[1] = make_float4(A[4], A[5], B[0], B[1]);
                    q[2] = make_float4(B[2], B[3], B[4], B[5]);
                    q[3] = make_float4(i2f(entry[a]), i2f(entry[b]), 0.0f, 0.0f);
                    const float w[12] = {A[0], A[1], A[2], A[3], A[4], A[5], B[0], B[1], B[2], B[3], B[4], B[5]};
                    if (!boxes_ordered(w)) unordered = true;
                } else {
                    const int first = m.node_leaf_first[i], count = m.node_leaf_count[i];
                    for (int k = 0; k < count; k++) {
                        const int t = m.leaf_indices[first + k];
                        if (t < 0 || t >= m.num_triangles) { rc = RT_E_INVALID; break; }
                        const float* v = m.vertices + 9 * (size_t)t;
                        const float* nn = m.normals + 3 * (size_t)t;
                        const float* uv = m.uvs + 6 * (size_t)t;
                        V3 v0 = v3(v[0], v[1], v[2]), v1 = v3(v[3], v[4], v[5]), v2 = v3(v[6], v[7], v[8]);
                        V3 e0 = v2 - v0, e1 = v1 - v0;                      // TrianglePrimitive.hpp:154-155
                        float d00 = dot(e0, e0), d01 = dot(e0, e1), d11 = dot(e1, e1);
                        float inv = 1.0f / (d00 * d11 - d01 * d01);        // TrianglePrimitive.hpp:164
                        records.push_back(make_float4(v0.x, v0.y, v0.z, nn[0]));
                        records.push_back(make_float4(nn[1], nn[2], e0.x, e0.y));
                        records.push_back(make_float4(e0.z, e1.x, e1.y, e1.z));
                        records.push_back(make_float4(d00, d01, d11, inv));
                        for (int c = 0; c < 6; c++) {
                            tri_uv.push_back(uv[c]);
                            if (!(fabsf(uv[c]) < 1e37f)) exact_uv = true;  // also catches NaN / inf
                        }
                        tri_id.push_back(t);
                        leaf_count.push_back(k == 0 ? count : 0);
                    }
                }
            }
            if (rc != RT_OK) break;
            // unused slots of the mesh's part
            const size_t vec_end = (size_t)slot_base + (size_t)slot_cap - skipped;
            records.resize(vec_end * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            tri_uv.resize(vec_end * 6, 0.0f);
            tri_id.resize(vec_end, -1);
            leaf_count.resize(vec_end, 0);
            segments.push_back({(size_t)node_base, vec_first, vec_end - vec_first});
            s->mesh_root_ref.push_back(entry[0]);
            s->mesh_exact_uv.push_back(exact_uv ? 1 : 0);
            mesh_flags.push_back(unordered ? kBoxUnordered : 0);
            {
                RtScene::MeshRefit rf;
                rf.node_base = (int32_t)node_base; rf.int_cap = (int32_t)int_cap; rf.slot_cap = (int32_t)slot_cap; rf.levels = max_level;
                rf.slot_base = (int32_t)slot_base; rf.num_slots = (int32_t)n_slot; rf.num_triangles = m.num_triangles;
                std::vector<std::vector<int32_t>> by_level((size_t)max_level + 1);
                for (int i = 0; i < m.num_nodes; i++)
                    if (m.node_children[2 * i] > 0) by_level[(size_t)level[i]].push_back(entry[i]);
                for (int l = max_level; l >= 1; l--) {
                    if (by_level[(size_t)l].empty()) continue;
                    rf.sched.insert(rf.sched.end(), by_level[(size_t)l].begin(), by_level[(size_t)l].end());
                    rf.level_end.push_back((int32_t)rf.sched.size());
                }
                s->mesh_refit.push_back(std::move(rf));
            }
        }
        if (rc == RT_OK) {
            s->num_materials = desc->num_materials;
            for (int i = 0; i < desc->num_instances; i++)
                if (!instance_ok(desc->instances[i], *s)) { rc = RT_E_INVALID; break; }
            for (int i = 0; i < desc->num_materials; i++) {
                const RtMaterialDesc& m = desc->materials[i];
                if (m.texture && (m.texture_width <= 0 || m.texture_height <= 0 || m.texture_pitch < (size_t)m.texture_width * 3)) { rc = RT_E_INVALID; break; }
            }
        }
    } catch (const std::bad_alloc&) {
        rc = RT_E_NOMEM;
    }
    if (rc != RT_OK) { delete s; return rc; }

    // ---- device upload ----
    auto fail = [&](int code) { rt_scene_destroy(s); return code; };
    hipError_t he = hipGetDevice(&s->device);
    if (he != hipSuccess) return fail(he == hipErrorNoDevice ? RT_E_NODEVICE : (int)he);
    {
        // the arrays start as what unused records hold -- zeros, triangle id -1 -- plus four padding records (a leaf's last iteration
        // looks one record ahead); the parts of meshes that came with a tree are copied over that
        const size_t total = records.size() / 4 + skipped;
        auto make = [&](void** d, size_t bytes, int byte_value) -> hipError_t {
            hipError_t e = hipMalloc(d, std::max<size_t>(bytes, 1));
            if (e == hipSuccess && bytes) e = hipMemset(*d, byte_value, bytes);
            if (e == hipSuccess) s->device_bytes += std::max<size_t>(bytes, 1);
            return e;
        };
        if ((he = make((void**)&s->d_records, (total + 1) * 4 * sizeof(float4), 0)) != hipSuccess) return fail((int)he);
        s->records_bytes = s->records_alloc_bytes = (total + 1) * 4 * sizeof(float4);
        if ((he = make((void**)&s->d_tri_uv, total * 6 * sizeof(float), 0)) != hipSuccess) return fail((int)he);
        if ((he = make((void**)&s->d_tri_id, total * sizeof(int32_t), 0xff)) != hipSuccess) return fail((int)he);
        if ((he = make((void**)&s->d_leaf_count, total * sizeof(int32_t), 0)) != hipSuccess) return fail((int)he);
        for (const Segment& g : segments) {
            if (g.count == 0) continue;
            he = hipMemcpy(s->d_records + g.dev_first * 4, records.data() + g.vec_first * 4, g.count * 4 * sizeof(float4), hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(s->d_tri_uv + g.dev_first * 6, tri_uv.data() + g.vec_first * 6, g.count * 6 * sizeof(float), hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(s->d_tri_id + g.dev_first, tri_id.data() + g.vec_first, g.count * sizeof(int32_t), hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(s->d_leaf_count + g.dev_first, leaf_count.data() + g.vec_first, g.count * sizeof(int32_t), hipMemcpyHostToDevice);
            if (he != hipSuccess) return fail((int)he);
        }
    }
    if ((rc = upload(&s->d_mesh_flags, mesh_flags, s->device_bytes))) return fail(rc);
    for (auto& rf : s->mesh_refit) {
        std::vector<int32_t> sched(rf.sched);
        sched.resize((size_t)std::max(rf.int_cap, 1), 0);            // (capacity for the schedule of any tree over the mesh)
        if ((rc = upload(&rf.d_sched, sched, s->device_bytes))) return fail(rc);
    }
    for (int mi : build_on_device) {                             // trees the device builds in place (before the instances take their root entries)
        const RtMeshDesc& m = desc->meshes[mi];
        const size_t n = (size_t)m.num_triangles;
        float* d = nullptr;
        he = hipMalloc((void**)&d, std::max<size_t>(n, 1) * 18 * sizeof(float));
        if (he != hipSuccess) return fail((int)he);
        if (n) {
            he = hipMemcpy(d, m.vertices, n * 9 * sizeof(float), hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(d + n * 9, m.normals, n * 3 * sizeof(float), hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(d + n * 12, m.uvs, n * 6 * sizeof(float), hipMemcpyHostToDevice);
        }
        rc = he != hipSuccess ? (int)he : rt_scene_rebuild_mesh_device(s, mi, d, d + n * 9, d + n * 12, (int32_t)n, nullptr);
        (void)hipFree(d);
        if (rc) return fail(rc);
    }
    std::vector<DevMaterial> mats((size_t)desc->num_materials);
    for (int i = 0; i < desc->num_materials; i++) {
        const RtMaterialDesc& m = desc->materials[i];
        DevMaterial& d = mats[i];
        memset(&d, 0, sizeof d);
        d.albedo[0] = m.albedo[0]; d.albedo[1] = m.albedo[1]; d.albedo[2] = m.albedo[2];
        d.roughness = m.roughness; d.metallic = m.metallic;
        if (m.texture && m.texture_width > 0) {
            // tight device copy (the reference uses cudaMallocPitch + GpuMat::upload, Material.hpp:35-41)
            const size_t row = (size_t)m.texture_width * 3, bytes = row * (size_t)m.texture_height;
            uint8_t* dt = nullptr;
            he = hipMalloc((void**)&dt, bytes);
            if (he != hipSuccess) return fail((int)he);
            s->d_textures.push_back(dt);
            he = hipMemcpy2D(dt, row, m.texture, m.texture_pitch, row, (size_t)m.texture_height, hipMemcpyHostToDevice);
            if (he != hipSuccess) return fail((int)he);
            s->device_bytes += bytes;
            d.texture = dt; d.texture_width = m.texture_width; d.texture_height = m.texture_height; d.texture_pitch = (uint32_t)row;
        }
    }
    if ((rc = upload(&s->d_materials, mats, s->device_bytes))) return fail(rc);
    for (int i = 0; i < desc->num_instances; i++) s->instances.push_back(make_dev_instance(desc->instances[i], *s));
    if ((rc = upload(&s->d_instances, s->instances, s->device_bytes))) return fail(rc);
    *out = s;
    return RT_OK;
}

#define RT_SCENE_CALL(s) if (!(s)) return RT_E_INVALID; std::lock_guard<std::recursive_mutex> scene_call_guard_((s)->call_mu)

int rt_scene_update_instance(RtScene* s, int32_t index, const RtInstanceDesc* instance)
{
    RT_SCENE_CALL(s);
    if (!s || !instance || index < 0 || index >= (int)s->instances.size() || !instance_ok(*instance, *s)) return RT_E_INVALID;
    s->instances[index] = make_dev_instance(*instance, *s);
    RT_HIP(hipMemcpy(s->d_instances + index, &s->instances[index], sizeof(DevInstance), hipMemcpyHostToDevice));
    return RT_OK;
}

int rt_scene_update_instance_async(RtScene* s, int32_t index, const RtInstanceDesc* instance, void* stream)
{
    RT_SCENE_CALL(s);
    if (!s || !instance || index < 0 || index >= (int)s->instances.size() || !instance_ok(*instance, *s)) return RT_E_INVALID;
    s->instances[index] = make_dev_instance(*instance, *s);
    hipLaunchKernelGGL(set_instance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, s->d_instances + index, s->instances[index]);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

namespace {
int refit_mesh(RtScene* s, int32_t mesh_index, const float* vertices, const float* normals, int32_t num_triangles, void* stream, bool on_device)
{
    RT_SCENE_CALL(s);
    if (!vertices || !normals || mesh_index < 0 || mesh_index >= (int)s->mesh_refit.size()) return RT_E_INVALID;
    const RtScene::MeshRefit& rf = s->mesh_refit[(size_t)mesh_index];
    if (num_triangles != rf.num_triangles) return RT_E_INVALID;
    if (rf.num_triangles == 0) return RT_OK;
    hipStream_t st = (hipStream_t)stream;
    const float* d_v = vertices;
    const float* d_n = normals;
    if (!on_device) {
        const size_t nv = (size_t)rf.num_triangles * 9, nn = (size_t)rf.num_triangles * 3, need = (nv + nn) * sizeof(float);
        if (s->refit_scratch_bytes < need) {
            (void)hipFree(s->d_refit_scratch);                  // (synchronises with a refit still in flight)
            s->d_refit_scratch = nullptr; s->refit_scratch_bytes = 0;
            RT_HIP(hipMalloc((void**)&s->d_refit_scratch, need));
            s->refit_scratch_bytes = need;
        }
        // (behind the previous host-array refit's last read of the scratch when that one ran on another stream; see RtScene)
        if (s->refit_scratch_done && s->refit_scratch_stream != st) RT_HIP(hipStreamWaitEvent(st, s->refit_scratch_done, 0));
        // (the host arrays may be pageable: the copies return once the bytes are staged, and stay ordered on the stream)
        RT_HIP(hipMemcpyAsync(s->d_refit_scratch, vertices, nv * sizeof(float), hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(s->d_refit_scratch + nv, normals, nn * sizeof(float), hipMemcpyHostToDevice, st));
        d_v = s->d_refit_scratch;
        d_n = s->d_refit_scratch + nv;
    }
    hipLaunchKernelGGL(refit_triangles_kernel, dim3((unsigned)((rf.num_slots + 255) / 256)), dim3(256), 0, st, s->d_records, s->d_tri_id,
                       rf.slot_base, rf.num_slots, d_v, d_n);
    // deepest level first: children before parents.  A wide level is a launch of its own; consecutive levels of at most
    // kRefitRunThreads nodes share one single-workgroup launch (a 28-level tree: 10 launches instead of 28 -- with the arrays
    // already on the device the call is launch-bound)
    int begin = 0;
    int32_t* mesh_flag = s->d_mesh_flags + mesh_index;
    // every interior record of the mesh is rewritten below, so the flag is decided anew: one frame with a NaN vertex in a deforming
    // mesh no longer keeps the mesh on the generic slab loop (4-7 % slower on c2) until its next rebuild
    RT_HIP(hipMemsetAsync(mesh_flag, 0, sizeof(int32_t), st));
    RefitRun run;
    run.levels = 0;
    auto flush = [&] {
        if (run.levels == 0) return;
        if (run.levels == 1)
            hipLaunchKernelGGL(refit_level_kernel, dim3((unsigned)((run.bound[1] - run.bound[0] + 255) / 256)), dim3(256), 0, st, s->d_records, s->d_tri_id,
                               s->d_leaf_count, d_v, rf.d_sched, run.bound[0], run.bound[1], mesh_flag);
        else
            hipLaunchKernelGGL(refit_run_kernel, dim3(1), dim3(kRefitRunThreads), 0, st, s->d_records, s->d_tri_id, s->d_leaf_count, d_v, rf.d_sched, run, mesh_flag);
        run.levels = 0;
    };
    for (int32_t end : rf.level_end) {
        if (end - begin > kRefitRunThreads) {
            flush();
            hipLaunchKernelGGL(refit_level_kernel, dim3((unsigned)((end - begin + 255) / 256)), dim3(256), 0, st, s->d_records, s->d_tri_id,
                               s->d_leaf_count, d_v, rf.d_sched, begin, end, mesh_flag);
        } else {
            if (run.levels == kRefitRunLevels) flush();
            if (run.levels == 0) run.bound[0] = begin;
            run.bound[++run.levels] = end;
        }
        begin = end;
    }
    flush();
    RT_HIP(hipGetLastError());
    if (!on_device) {                                           // the last read of the scratch has been queued
        if (!s->refit_scratch_done) RT_HIP(hipEventCreateWithFlags(&s->refit_scratch_done, hipEventDisableTiming));
        RT_HIP(hipEventRecord(s->refit_scratch_done, st));
        s->refit_scratch_stream = st;
    }
    return RT_OK;
}
}  // namespace

int rt_scene_refit_mesh(RtScene* s, int32_t mesh_index, const float* vertices, const float* normals, int32_t num_triangles, void* stream)
{
    return refit_mesh(s, mesh_index, vertices, normals, num_triangles, stream, false);
}

int rt_scene_refit_mesh_device(RtScene* s, int32_t mesh_index, const float* d_vertices, const float* d_normals, int32_t num_triangles, void* stream)
{
    return refit_mesh(s, mesh_index, d_vertices, d_normals, num_triangles, stream, true);
}

int rt_scene_debug_read(RtScene* s, int32_t which, void* host_dst, size_t capacity, size_t* bytes)
{
    RT_SCENE_CALL(s);
    if (!bytes || which < 0 || which > 4) return RT_E_INVALID;
    size_t recs = 4;                                            // the padding records at the end
    for (const auto& rf : s->mesh_refit) recs = std::max(recs, (size_t)rf.slot_base + (size_t)rf.slot_cap + 4);
    recs -= 4;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
    case 0: src = s->d_records; n = (recs + 1) * 4 * sizeof(float4); break;       // (+ the four padding float4 = one record)
    case 1: src = s->d_tri_uv; n = recs * 6 * sizeof(float); break;
    case 2: src = s->d_tri_id; n = recs * sizeof(int32_t); break;
    case 3: src = s->d_leaf_count; n = recs * sizeof(int32_t); break;
    default: src = s->d_instances; n = s->instances.size() * sizeof(DevInstance); break;
    }
    *bytes = n;
    if (!host_dst || capacity < n) return RT_OK;
    RT_HIP(hipDeviceSynchronize());
    if (n) RT_HIP(hipMemcpy(host_dst, src, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_destroy(RtScene* s)
{
    if (!s) return RT_OK;
    for (int k = 0; k < 2; k++) {
        if (s->overlap.stream[k]) { (void)hipStreamSynchronize(s->overlap.stream[k]); (void)hipStreamDestroy(s->overlap.stream[k]); }
        if (s->overlap.done[k]) (void)hipEventDestroy(s->overlap.done[k]);
    }
    if (s->order.sort_stream) (void)hipStreamSynchronize(s->order.sort_stream);
    for (auto& o : s->order.entry) {
        if (o.sort_done) { (void)hipEventDestroy(o.sort_done); for (auto& e : o.seen) (void)hipEventDestroy(e.done); }
        (void)hipFree(o.d_cost);
    }
    if (s->order.sort_stream) (void)hipStreamDestroy(s->order.sort_stream);
    for (auto& rf : s->mesh_refit) (void)hipFree(rf.d_sched);
    if (s->refit_scratch_done) (void)hipEventDestroy(s->refit_scratch_done);
    (void)hipFree(s->d_refit_scratch);
    (void)hipFree(s->d_ex_scratch);
    for (auto& sl : s->view.slot) { if (sl.done) (void)hipEventDestroy(sl.done); (void)hipFree(sl.d_dirs); }
    (void)hipFree(s->d_records); (void)hipFree(s->d_tri_uv); (void)hipFree(s->d_tri_id);
    (void)hipFree(s->d_leaf_count); (void)hipFree(s->d_mesh_flags); (void)hipFree(s->d_instances); (void)hipFree(s->d_materials);
    for (uint8_t* t : s->d_textures) (void)hipFree(t);
    delete s;
    return RT_OK;
}

int rt_scene_info(const RtScene* s, size_t* device_bytes, int32_t* max_stack)
{
    if (!s) return RT_E_INVALID;
    if (device_bytes) *device_bytes = s->device_bytes;
    if (max_stack) *max_stack = s->max_stack;
    return RT_OK;
}

int rt_scene_view_stats(RtScene* s, uint64_t* launches, uint64_t* fallbacks, uint64_t* grows, int32_t* slot_frames)
{
    RT_SCENE_CALL(s);
    std::lock_guard<std::mutex> lock(s->view.m);
    if (launches) *launches = s->view.launches;
    if (fallbacks) *fallbacks = s->view.fallbacks;
    if (grows) *grows = s->view.grows;
    if (slot_frames) *slot_frames = s->view.slot_frames;
    return RT_OK;
}

int rt_scene_view_cull_stats(RtScene* s, int32_t* frames, uint64_t* culled_leaves)
{
    RT_SCENE_CALL(s);
    if (!frames || !culled_leaves) return RT_E_INVALID;
    *frames = 0;
    const RtScene::ViewPool::Written w = s->view.written;
    if (!w.culled || w.frames < 1 || w.frames > kMaxBatch || s->view.slot_frames < 1) return RT_OK;
    RT_HIP(hipDeviceSynchronize());                             // (the pre-pass that wrote them, and nothing writes them meanwhile: call_mu)
    unsigned long long* d_out = nullptr;
    RT_HIP(hipMalloc((void**)&d_out, sizeof(unsigned long long) * kMaxBatch));
    hipError_t e = hipMemset(d_out, 0, sizeof(unsigned long long) * kMaxBatch);
    for (int i = 0; i < w.n && e == hipSuccess; i++) {
        if (w.count[i] < 1) continue;
        hipLaunchKernelGGL(view_cull_count_kernel, dim3((unsigned)((w.count[i] + 255) / 256), (unsigned)w.frames), dim3(256), 0, nullptr,
                           s->d_records, w.view_base, (uint32_t)((size_t)s->view.frame_records * 64), w.first[i], w.count[i], d_out);
        e = hipGetLastError();
    }
    unsigned long long host[kMaxBatch] = {};
    if (e == hipSuccess) e = hipMemcpy(host, d_out, sizeof(host), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return (int)e;
    for (int k = 0; k < w.frames; k++) culled_leaves[k] = host[k];
    *frames = w.frames;
    return RT_OK;
}

int rt_scene_dir_table_stats(RtScene* s, uint64_t out[4])
{
    RT_SCENE_CALL(s);
    if (!out) return RT_E_INVALID;
    std::lock_guard<std::mutex> lock(s->view.m);
    out[0] = s->view.dir_launches; out[1] = s->view.dir_skipped; out[2] = s->view.dir_grows; out[3] = s->view.dir_bytes;
    return RT_OK;
}

int rt_scene_reserve_views(RtScene* s, int32_t frames_per_launch)
{
    RT_SCENE_CALL(s);
    if (frames_per_launch < 0 || frames_per_launch > kMaxBatch) return RT_E_INVALID;
    RtScene::ViewPool& v = s->view;
    view_decide(s);
    if (!view_mode() || !v.usable) return RT_E_INVALID;         // (more than eight instances, or no interior records: this scene renders without views)
    if (frames_per_launch == 0) { v.reserved = false; return RT_OK; }      // back to growing on demand (what is there stays)
    if (frames_per_launch != v.slot_frames) {
        const int rc = view_resize(s, frames_per_launch);
        if (rc) return rc;
    }
    v.reserved = true;
    return RT_OK;
}

int rt_scene_memory(RtScene* s, size_t* records_bytes, size_t* view_pool_bytes, size_t* device_bytes, int32_t* view_slots, int32_t* view_slot_frames)
{
    RT_SCENE_CALL(s);
    if (records_bytes) *records_bytes = s->records_bytes;
    if (view_pool_bytes) *view_pool_bytes = s->view.slot_frames > 0 ? (size_t)s->view.frame_records * 64 * (size_t)s->view.slots * (size_t)s->view.slot_frames : 0;
    if (device_bytes) *device_bytes = s->device_bytes;
    if (view_slots) *view_slots = s->view.slots;
    if (view_slot_frames) *view_slot_frames = s->view.slot_frames;
    return RT_OK;
}

int rt_scene_mesh_flags(RtScene* s, int32_t mesh_index, int32_t* flags)
{
    if (!s || !flags || mesh_index < 0 || mesh_index >= (int)s->mesh_refit.size()) return RT_E_INVALID;
    RT_HIP(hipMemcpy(flags, s->d_mesh_flags + mesh_index, sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_mesh_capacity(const RtScene* s, int32_t mesh_index, int32_t* max_triangles)
{
    if (!s || !max_triangles || mesh_index < 0 || mesh_index >= (int)s->mesh_refit.size()) return RT_E_INVALID;
    const RtScene::MeshRefit& rf = s->mesh_refit[(size_t)mesh_index];
    *max_triangles = std::min(rf.slot_cap, rf.int_cap + 1);
    return RT_OK;
}

// (every render entry point: the scene's call_mu is held while the launch is prepared and queued; a wait the caller asked for
// happens after it has been released)
#define RT_WAIT_IF(synchronize, stream) do { if (synchronize) RT_HIP(hipStreamSynchronize((hipStream_t)(stream))); } while (0)

int rt_render_batch(RtScene* s, const RtCameraParams* cams, uint8_t* const* d_imgs, size_t pitch, int32_t count,
                    void* stream, int synchronize)
{
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cams, d_imgs, count, pitch);
        if (rc) return rc;
        if ((rc = launch(p, false, (hipStream_t)stream, 0, s))) return rc;
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_scene_loop_stats(RtScene* s, const RtCameraParams* cams, uint8_t* const* d_imgs, size_t pitch, int32_t count, void* stream, uint64_t* stats)
{
    if (!stats) return RT_E_INVALID;
    RT_SCENE_CALL(s);
    RenderParams p;
    int rc = fill_params(p, s, cams, d_imgs, count, pitch);
    if (rc) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    unsigned long long* d = nullptr;
    RT_HIP(hipMalloc((void**)&d, RT_LOOP_WORDS * sizeof(uint64_t)));
    hipError_t e = hipMemsetAsync(d, 0, RT_LOOP_WORDS * sizeof(uint64_t), (hipStream_t)stream);
    p.loop_stats = d;
    if (e == hipSuccess) rc = launch(p, false, (hipStream_t)stream, 1, s, true);
    if (e == hipSuccess && rc == RT_OK) e = hipMemcpy(stats, d, RT_LOOP_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e != hipSuccess ? (int)e : rc;
}

int rt_render(RtScene* s, const RtCameraParams* cam, uint8_t* d_img, size_t pitch, void* stream, int synchronize)
{
    return rt_render_batch(s, cam, &d_img, pitch, 1, stream, synchronize);
}

// Camera::render_scene(scene, img, pitch, synchronize = false) on the default stream (Camera.cu:18-41) -- see rt_hip.h.
int rt_render_overlapped(RtScene* s, const RtCameraParams* cam, uint8_t* d_img, size_t pitch)
{
    RT_SCENE_CALL(s);
    RenderParams p;
    int rc = fill_params(p, s, cam, &d_img, 1, pitch);
    if (rc) return rc;
    static const bool enabled = [] { const char* e = getenv("RT_RENDER_OVERLAP"); return !(e && e[0] == '0'); }();
    if (!enabled) return launch(p, false, nullptr, 0, s);
    RtScene::Overlap& ov = s->overlap;
    std::lock_guard<std::mutex> lock(ov.m);
    if (!ov.stream[0]) {
        // hipStreamDefault = a BLOCKING stream: work on the null stream waits for everything issued here before it, and
        // everything issued here waits for earlier null-stream work -- the ordering a default-stream launch has with the
        // caller's copies, memsets, instance updates and hipDeviceSynchronize
        // Round 6: stream 0 has the HIGHER priority.  The reference's loop issues two frames and then synchronises the device: two
        // equal streams share the chip, both frames run at half speed and END TOGETHER -- their tails coincide and nothing is hidden
        // (two overlapped frames 245 us, each alone 125: rocprofv3 timeline in profiles/r06_experiments/single_frame_gap.md).  With
        // priorities the first frame of a pair takes the chip, the second fills the slots its tail leaves free and then runs alone:
        // one tail exposed instead of two.  (RT_OVERLAP_PRIORITY=0: two equal streams, for the A/B.)
        static const bool prio = [] { const char* e = getenv("RT_OVERLAP_PRIORITY"); return !(e && e[0] == '0'); }();
        int least = 0, greatest = 0;
        if (!prio || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        hipStream_t st[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        hipError_t e = hipStreamCreateWithPriority(&st[0], hipStreamDefault, greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&st[1], hipStreamDefault, least);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[0], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[1], hipEventDisableTiming);
        if (e != hipSuccess) {
            for (int k = 0; k < 2; k++) { if (st[k]) (void)hipStreamDestroy(st[k]); if (ev[k]) (void)hipEventDestroy(ev[k]); }
            return (int)e;
        }
        for (int k = 0; k < 2; k++) { ov.stream[k] = st[k]; ov.done[k] = ev[k]; }
    }
    const RtScene::Overlap::Range r{(uintptr_t)d_img, (uintptr_t)d_img + (size_t)(p.height - 1) * pitch + (size_t)p.width * 3};
    auto meets = [&](const std::vector<RtScene::Overlap::Range>& v) {
        for (const auto& w : v) if (w.lo < r.hi && r.lo < w.hi) return true;
        return false;
    };
    // (the high-priority stream takes the frame whenever it is idle -- after every synchronise, so the first frame of a pair)
    int use = ov.next;
    if (use == 1) { if (hipStreamQuery(ov.stream[0]) == hipSuccess) use = 0; else (void)hipGetLastError(); }
    int other = use ^ 1;
    const bool hit_other = meets(ov.written[other]);
    if (hit_other && !meets(ov.written[use])) {
        std::swap(use, other);                                  // same image as the frame in flight over there: stream order does it
    } else if (hit_other) {
        RT_HIP(hipEventRecord(ov.done[other], ov.stream[other]));          // (recorded when it is needed: after everything issued there so far)
        RT_HIP(hipStreamWaitEvent(ov.stream[use], ov.done[other], 0));
        ov.written[other].clear();                              // everything issued there so far is now ordered before this stream's next work
        ov.waits++;
    }
    rc = launch(p, false, ov.stream[use], 0, s);
    if (rc) return rc;
    std::vector<RtScene::Overlap::Range>& mine = ov.written[use];
    bool known = false;
    for (const auto& w : mine) known = known || (w.lo == r.lo && w.hi == r.hi);
    if (!known) {
        if (mine.size() >= 8) {                                 // an application cycling through many images: one hull (may over-order, never under)
            RtScene::Overlap::Range hull = r;
            for (const auto& w : mine) { hull.lo = std::min(hull.lo, w.lo); hull.hi = std::max(hull.hi, w.hi); }
            mine.assign(1, hull);
        } else {
            mine.push_back(r);
        }
    }
    ov.launches++;
    ov.next = use ^ 1;
    return RT_OK;
}

int rt_render_overlapped_stats(const RtScene* s, uint64_t* launches, uint64_t* cross_stream_waits)
{
    if (!s) return RT_E_INVALID;
    if (launches) *launches = s->overlap.launches;
    if (cross_stream_waits) *cross_stream_waits = s->overlap.waits;
    return RT_OK;
}

int rt_render_ids(RtScene* s, const RtCameraParams* cam, uint8_t* d_img, size_t pitch, int32_t* d_hit_instance,
                  int32_t* d_hit_triangle, void* stream, int synchronize)
{
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cam, &d_img, 1, pitch);
        if (rc) return rc;
        p.hit_instance = d_hit_instance; p.hit_triangle = d_hit_triangle;
        if ((rc = launch(p, false, (hipStream_t)stream, 0, s))) return rc;   // (with the scene: the kernel whose ids are checked is the one that is timed, views included)
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

// rt_render_gbuffer and rt_render_gbuffer_table (table: the caller's ray table, non-null; null = the cameras' own rays)
static int render_gbuffer(RtScene* s, const RtRayTable* table, const RtCameraParams* cams, int32_t count, uint8_t* const* d_imgs, size_t pitch,
                          const RtGBuffer* out, void* stream, int synchronize)
{
    // (every argument is judged before the scene is touched)
    if (!s || !cams || !out || count < 1 || count > kMaxBatch || !camera_ok(&cams[0])) return RT_E_INVALID;
    for (int i = 1; i < count; i++) if (cams[i].width != cams[0].width || cams[i].height != cams[0].height) return RT_E_INVALID;
    const bool planes = out->t || out->depth || out->instance || out->triangle || out->location || out->normal || out->uv;
    if (!planes && !d_imgs) return RT_E_INVALID;
    if (d_imgs) {
        if (pitch < (size_t)cams[0].width * 3) return RT_E_INVALID;
        for (int i = 0; i < count; i++) if (!d_imgs[i]) return RT_E_INVALID;
    }
    // (the table is looked at last: whatever can be judged without it has been)
    if (table && (cams[0].width != table->width || cams[0].height != table->height)) return RT_E_INVALID;
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cams, d_imgs, count, pitch, d_imgs == nullptr);
        if (rc) return rc;
        GBufParams g;
        g.t = out->t; g.depth = out->depth; g.instance = out->instance; g.triangle = out->triangle;
        g.location = out->location; g.normal = out->normal; g.uv = out->uv;
        for (int i = 0; i < kMaxBatch; i++) {
            const RtCameraParams& c = cams[i < count ? i : 0];
            g.q_pose[i] = euler2quat(v3(c.camera_pose[3], c.camera_pose[4], c.camera_pose[5]));
        }
        if ((rc = launch_gbuffer(s, p, g, (hipStream_t)stream, table ? table->d_table : nullptr))) return rc;
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_render_gbuffer(RtScene* s, const RtCameraParams* cams, int32_t count, uint8_t* const* d_imgs, size_t pitch, const RtGBuffer* out,
                      void* stream, int synchronize)
{
    return render_gbuffer(s, nullptr, cams, count, d_imgs, pitch, out, stream, synchronize);
}

int rt_render_gbuffer_table(RtScene* s, const RtRayTable* table, const RtCameraParams* poses, int32_t count, uint8_t* const* d_imgs, size_t pitch,
                            const RtGBuffer* out, void* stream, int synchronize)
{
    if (!table) return RT_E_INVALID;
    return render_gbuffer(s, table, poses, count, d_imgs, pitch, out, stream, synchronize);
}

// ---- rolling frames (include/rt_hip.h "rolling frames") --------------------------------------------------
extern "C++" {
namespace {
bool rolling_axis_ok(int32_t axis, int32_t slice_pixels) { return (axis == 0 || axis == 1) && slice_pixels >= 8 && slice_pixels % 8 == 0; }
bool rolling_shape(int32_t width, int32_t height, int32_t axis, int32_t slice_pixels, int32_t& slices)
{
    if (width < 1 || height < 1 || !rolling_axis_ok(axis, slice_pixels)) return false;
    const int32_t extent = axis ? height : width;
    slices = (int32_t)(((int64_t)extent + slice_pixels - 1) / slice_pixels);
    return true;
}
size_t rolling_record_bytes(int32_t count, int32_t slices)
{
    if (count < 1 || count > kMaxBatch || slices < 1) return 0;
    return ((size_t)count * (size_t)slices * sizeof(RollRecord) + 255) / 256 * 256;     // (whole 256-byte blocks, as the cloud workspace's parts)
}
// the records of count x slices poses: the host's quaternions, so that their bits are rt_ray_table_rays' and GBufParams::q_pose's
void rolling_pack(const RtRollingPose* poses, size_t n, std::vector<RollRecord>& rec)
{
    rec.resize(n);
    for (size_t k = 0; k < n; k++) {
        const RtRollingPose& ps = poses[k];
        RollRecord& o = rec[k];
        for (int a = 0; a < 3; a++) o.origin[a] = ps.camera_pose[a];
        o.pad = 0;
        o.q_cam = euler2quat(v3(ps.inv_camera_pose[3], ps.inv_camera_pose[4], ps.inv_camera_pose[5]));
        o.q_pose = euler2quat(v3(ps.camera_pose[3], ps.camera_pose[4], ps.camera_pose[5]));
    }
}
// The rolling render of `count` frames into the planes of g (and `d_local`), the records into `d_records` first, on `stream`.  Every
// argument has been judged.  The copy reads pageable host memory: it returns when the records have left `rec` (it may wait for work
// issued EARLIER on the stream, never for the launch that follows it).
int rolling_render(RtScene* s, const RtRayTable* table, const RtRollingPose* poses, int32_t count, int32_t slices, int32_t axis,
                   int32_t slice_pixels, uint8_t* const* d_imgs, size_t pitch, GBufParams& g, float* d_local, void* d_records, hipStream_t st)
{
    std::vector<RollRecord> rec;
    rolling_pack(poses, (size_t)count * (size_t)slices, rec);
    RT_HIP(hipMemcpyAsync(d_records, rec.data(), rec.size() * sizeof(RollRecord), hipMemcpyHostToDevice, st));
    RtCameraParams cams[kMaxBatch];
    memset(cams, 0, sizeof cams);
    for (int i = 0; i < count; i++) {                           // (the size and, for fill_params, the first slice's pose: the kernel reads the records)
        cams[i].width = table->width; cams[i].height = table->height;
        memcpy(cams[i].camera_pose, poses[(size_t)i * slices].camera_pose, sizeof cams[i].camera_pose);
        memcpy(cams[i].inv_camera_pose, poses[(size_t)i * slices].inv_camera_pose, sizeof cams[i].inv_camera_pose);
    }
    RollParams r;
    r.records = (const RollRecord*)d_records; r.local = d_local; r.slices = slices; r.axis = axis; r.slice_tiles = slice_pixels / kPrimTile;
    RT_SCENE_CALL(s);                                           // (held for the launch only)
    RenderParams p;
    int rc = fill_params(p, s, cams, d_imgs, count, pitch, d_imgs == nullptr);
    if (rc) return rc;
    return launch_gbuffer_rolling(p, g, r, st, table->d_table);
}
}  // namespace
}  // extern "C++"

int rt_rolling_slices(int32_t width, int32_t height, int32_t axis, int32_t slice_pixels, int32_t* slices)
{
    int32_t n = 0;
    if (!slices || !rolling_shape(width, height, axis, slice_pixels, n)) return RT_E_INVALID;
    *slices = n;
    return RT_OK;
}

size_t rt_rolling_workspace_bytes(int32_t count, int32_t slices) { return rolling_record_bytes(count, slices); }

int rt_render_gbuffer_rolling(RtScene* s, const RtRayTable* table, const RtRollingPose* poses, int32_t count, int32_t axis, int32_t slice_pixels,
                              uint8_t* const* d_imgs, size_t pitch, const RtGBuffer* out, float* d_local, void* d_workspace,
                              size_t workspace_bytes, void* stream, int synchronize)
{
    // (every argument is judged before any device call)
    int32_t slices = 0;
    if (!s || !table || !poses || !out || !d_workspace || count < 1 || count > kMaxBatch || !rolling_axis_ok(axis, slice_pixels)) return RT_E_INVALID;
    const bool planes = out->t || out->depth || out->instance || out->triangle || out->location || out->normal || out->uv || d_local;
    if (!planes && !d_imgs) return RT_E_INVALID;
    if (d_imgs) for (int i = 0; i < count; i++) if (!d_imgs[i]) return RT_E_INVALID;
    // (the table is looked at last: whatever can be judged without it has been)
    if (!rolling_shape(table->width, table->height, axis, slice_pixels, slices) || workspace_bytes < rolling_record_bytes(count, slices)) return RT_E_INVALID;
    if (d_imgs && pitch < (size_t)table->width * 3) return RT_E_INVALID;
    GBufParams g;
    memset(&g, 0, sizeof g);                                    // (q_pose: not read, the records carry it)
    g.t = out->t; g.depth = out->depth; g.instance = out->instance; g.triangle = out->triangle;
    g.location = out->location; g.normal = out->normal; g.uv = out->uv;
    const int rc = rolling_render(s, table, poses, count, slices, axis, slice_pixels, d_imgs, pitch, g, d_local, d_workspace, (hipStream_t)stream);
    if (rc) return rc;
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_render_debug(RtScene* s, const RtCameraParams* cam, uint8_t* d_img, size_t pitch,
                    const RtDebugPlanes* planes, void* stream, int synchronize)
{
    if (!planes) return RT_E_INVALID;
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cam, &d_img, 1, pitch);
        if (rc) return rc;
        p.hit_instance = planes->hit_instance; p.hit_triangle = planes->hit_triangle; p.node_pops = planes->node_pops;
        p.aabb_tests = planes->aabb_tests; p.tri_tests = planes->tri_tests; p.inside_hits = planes->inside_hits;
        if ((rc = launch(p, true, (hipStream_t)stream, 0))) return rc;
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

// Samples are rendered in chunks of as many sample indices as fit the scratch budget: per chunk one
// render_ex_kernel launch with grid.y = chunk, then one resolve_ex_kernel.
constexpr size_t kExScratchBudget = (size_t)2 << 30;           // 16 B per path

static int ex_env_int(const char* name, int fallback)
{
    const char* e = getenv(name);
    return e && *e ? atoi(e) : fallback;
}

static int launch_ex(RtScene* s, RenderParams& p, const RtRenderOptions* opts, int32_t* d_total_pops, hipStream_t stream, int synchronize)
{
    if (!opts || opts->spp < 1 || opts->bounces < 0) return RT_E_INVALID;
    if (p.local_rows == 0) return RT_OK;
    p.spp = opts->spp; p.bounces = opts->bounces; p.lighting = opts->lighting ? 1 : 0; p.total_pops = d_total_pops;
    p.tiles_x = (p.width + kTile - 1) / kTile;
    p.tiles_y = (p.local_rows + kTile - 1) / kTile;
    const size_t npix = (size_t)p.local_rows * p.width;
    const size_t ntiles = (size_t)p.tiles_x * p.tiles_y;
    const char* trace_file = getenv("RT_TRACE_FILE");                               // diagnostics only: first chunk, per-lane form
    const bool simple = p.bounces == 0 && !p.lighting;
    // (read per call, not cached: the parity tests switch between the two mappings)
    // The samples of a pixel in one wave (render_ex_kernel<.., PX>): the default from four samples per pixel on.
    // RT_EX_PIXEL_WAVES=0 selects the older mapping (one sample index per launch row, sample planes + resolve pass).
    const bool pixel_waves = !trace_file && p.spp >= 4 && ex_env_int("RT_EX_PIXEL_WAVES", 1) != 0;
    if (pixel_waves) {
        const bool many = p.spp > 64;                                               // several launches: running sums in ex_acc
        const size_t need = many ? npix * sizeof(float4) : 0;
        if (s->ex_scratch_bytes < need) {
            (void)hipFree(s->d_ex_scratch);                                         // (synchronises with renders in flight)
            s->d_ex_scratch = nullptr; s->ex_scratch_bytes = 0;
            RT_HIP(hipMalloc((void**)&s->d_ex_scratch, need));
            s->ex_scratch_bytes = need;
        }
        p.ex_acc = s->d_ex_scratch;
        // (four LDS rows per lane hold a wave's samples for the in-wave sum, whatever the depth of the stack)
        const size_t lds = (size_t)std::max(lds_rows(p.stack_depth) + 1, 4) * kExBlock * sizeof(int);       // (+ the optimistic stack's spare row)
        // the samples-only kernel's rays all start at the camera: one view of the tree serves every sample of the frame
        const int view_slot = view_prepare(s, p, stream, p.spp);
        struct ViewDone {
            RtScene* s; int slot; hipStream_t stream;
            ~ViewDone() { view_done(s, slot, stream); }
        } view_guard{s, view_slot, stream};
        for (int base = 0; base < p.spp; base += 64) {
            const int n = std::min(64, p.spp - base);
            int slots = 4;
            while (slots < n) slots <<= 1;
            const int ppw = 64 / slots;                                             // pixels of a wave: 16, 8, 4, 2 or 1
            p.px_n = slots; p.px_count = n;
            p.px_pw = ppw >= 16 ? 4 : (ppw >= 4 ? 2 : (ppw >= 2 ? 2 : 1));
            p.px_ph = ppw / p.px_pw;
            p.px_first = base == 0 ? 1 : 0; p.px_last = base + n == p.spp ? 1 : 0;
            p.sample_base = base;
            p.tiles_x = (p.width + 2 * p.px_pw - 1) / (2 * p.px_pw);
            p.tiles_y = (p.local_rows + 2 * p.px_ph - 1) / (2 * p.px_ph);
            const dim3 grid((unsigned)((size_t)p.tiles_x * p.tiles_y * 4));         // four one-wave workgroups per tile
            if (simple && view_slot >= 0) hipLaunchKernelGGL((render_ex_kernel<true, true, true>), grid, dim3(kExBlock), lds, stream, p);
            else if (simple) hipLaunchKernelGGL((render_ex_kernel<true, true>), grid, dim3(kExBlock), lds, stream, p);
            else if (view_slot >= 0) hipLaunchKernelGGL((render_ex_kernel<false, true, true>), grid, dim3(kExBlock), lds, stream, p);
            else hipLaunchKernelGGL((render_ex_kernel<false, true>), grid, dim3(kExBlock), lds, stream, p);
            RT_HIP(hipGetLastError());
        }
        if (synchronize) RT_HIP(hipStreamSynchronize(stream));
        return RT_OK;
    }
    size_t budget = kExScratchBudget;
    if (const char* e = getenv("RT_EX_SCRATCH_BYTES")) budget = (size_t)strtoull(e, nullptr, 10);   // tests: force several chunks
    const size_t per_sample = npix * sizeof(float4);            // bytes per sample index: its plane of samples
    int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)p.spp, budget / per_sample, (size_t)65535}));    // (65535: grid.y)
    {                                                           // chunks of equal size
        const int nchunks = (p.spp + chunk - 1) / chunk;
        const int even = (p.spp + nchunks - 1) / nchunks;
        chunk = std::min(chunk, even);
    }
    const size_t need = (size_t)(chunk + 1) * npix * sizeof(float4);
    if (s->ex_scratch_bytes < need) {
        (void)hipFree(s->d_ex_scratch);                                             // (synchronises with renders in flight)
        s->d_ex_scratch = nullptr; s->ex_scratch_bytes = 0;
        RT_HIP(hipMalloc((void**)&s->d_ex_scratch, need));
        s->ex_scratch_bytes = need;
    }
    p.ex_acc = s->d_ex_scratch;
    p.ex_samples = s->d_ex_scratch + npix;
    const size_t lds_wave = (size_t)(lds_rows(p.stack_depth) + 1) * kExBlock * sizeof(int);         // (+ the optimistic stack's spare row)
    for (int base = 0; base < p.spp; base += chunk) {
        const int n = std::min(chunk, p.spp - base);
        p.sample_base = base;
        const dim3 grid((unsigned)ntiles * 4, (unsigned)n);                        // four one-wave workgroups per tile
        const size_t trace_n = (size_t)grid.x * grid.y * 16;
        const bool tracing = trace_file && base == 0;
        if (tracing) RT_HIP(trace_begin(p, trace_n));
        if (simple) hipLaunchKernelGGL(render_ex_kernel<true>, grid, dim3(kExBlock), lds_wave, stream, p);
        else hipLaunchKernelGGL(render_ex_kernel<false>, grid, dim3(kExBlock), lds_wave, stream, p);
        RT_HIP(hipGetLastError());
        if (tracing) RT_HIP(trace_end(p, trace_n, trace_file, stream));
        hipLaunchKernelGGL(resolve_ex_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, p, n, base == 0 ? 1 : 0,
                           base + n == p.spp ? 1 : 0);
        RT_HIP(hipGetLastError());
    }
    if (synchronize) RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

int rt_render_ex(RtScene* s, const RtCameraParams* cam, const RtRenderOptions* opts, uint8_t* d_img, size_t pitch,
                 int32_t* d_total_pops, void* stream, int synchronize)
{
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cam, &d_img, 1, pitch);
        if (rc) return rc;
        if ((rc = launch_ex(s, p, opts, d_total_pops, (hipStream_t)stream, 0))) return rc;
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_render_ex_stripes(RtScene* s, const RtCameraParams* cam, const RtRenderOptions* opts, uint8_t* d_local, size_t local_pitch,
                         int32_t stripe_rows, int32_t rank, int32_t num_ranks, void* stream, int synchronize)
{
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cam, &d_local, 1, local_pitch);
        if (rc) return rc;
        int32_t rows = 0;
        if ((rc = rt_stripe_rows(p.height, stripe_rows, rank, num_ranks, &rows))) return rc;
        p.local_rows = rows; p.stripe_rows = stripe_rows; p.rank = rank; p.num_ranks = num_ranks;
        p.frames[0].rank = rank; p.frames[0].local_rows = rows;
        if ((rc = launch_ex(s, p, opts, nullptr, (hipStream_t)stream, 0))) return rc;
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_stripe_rows(int32_t height, int32_t stripe_rows, int32_t rank, int32_t num_ranks, int32_t* rows)
{
    if (!rows || height < 0 || stripe_rows <= 0 || num_ranks <= 0 || rank < 0 || rank >= num_ranks) return RT_E_INVALID;
    int32_t n = 0;
    for (int32_t s0 = rank; (int64_t)s0 * stripe_rows < height; s0 += num_ranks)
        n += std::min(stripe_rows, height - s0 * stripe_rows);
    *rows = n;
    return RT_OK;
}

// frame i of the launch renders the stripes of owner (rank + first_frame + i) % num_ranks when first_frame >= 0, of `rank` otherwise
static int render_stripes_batch(RtScene* s, const RtCameraParams* cams, uint8_t* const* d_locals, size_t local_pitch, int32_t count,
                                int32_t stripe_rows, int32_t rank, int32_t num_ranks, int32_t first_frame, void* stream, int synchronize)
{
    {
    RT_SCENE_CALL(s);
    RenderParams p;
    int rc = fill_params(p, s, cams, d_locals, count, local_pitch);
    if (rc) return rc;
    int32_t rows = 0;
    if ((rc = rt_stripe_rows(p.height, stripe_rows, rank, num_ranks, &rows))) return rc;
    p.stripe_rows = stripe_rows; p.rank = rank; p.num_ranks = num_ranks;
    int32_t most = 0;
    for (int i = 0; i < count; i++) {
        FrameParams& f = p.frames[i];
        f.rank = first_frame >= 0 ? (int32_t)(((int64_t)rank + first_frame + i) % num_ranks) : rank;
        if (f.rank != rank) { if ((rc = rt_stripe_rows(p.height, stripe_rows, f.rank, num_ranks, &f.local_rows))) return rc; }
        else f.local_rows = rows;
        most = std::max(most, f.local_rows);
    }
    p.local_rows = most;                                        // the grid covers the tallest frame; shorter ones leave their last tiles empty
    if ((rc = launch(p, false, (hipStream_t)stream, 0, s))) return rc;
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_render_stripes_batch(RtScene* s, const RtCameraParams* cams, uint8_t* const* d_locals, size_t local_pitch, int32_t count,
                            int32_t stripe_rows, int32_t rank, int32_t num_ranks, void* stream, int synchronize)
{
    return render_stripes_batch(s, cams, d_locals, local_pitch, count, stripe_rows, rank, num_ranks, -1, stream, synchronize);
}

int rt_render_stripes_batch_rotating(RtScene* s, const RtCameraParams* cams, uint8_t* const* d_locals, size_t local_pitch, int32_t count,
                                     int32_t stripe_rows, int32_t rank, int32_t num_ranks, int32_t first_frame, void* stream, int synchronize)
{
    if (first_frame < 0) return RT_E_INVALID;
    return render_stripes_batch(s, cams, d_locals, local_pitch, count, stripe_rows, rank, num_ranks, first_frame, stream, synchronize);
}

int rt_render_stripes(RtScene* s, const RtCameraParams* cam, uint8_t* d_local, size_t local_pitch,
                      int32_t stripe_rows, int32_t rank, int32_t num_ranks, void* stream, int synchronize)
{
    return rt_render_stripes_batch(s, cam, &d_local, local_pitch, 1, stripe_rows, rank, num_ranks, stream, synchronize);
}

static int unstripe_batch(const uint8_t* d_gathered, size_t local_pitch, size_t rank_stride, size_t src_frame_stride,
                          uint8_t* d_imgs, size_t pitch, size_t dst_frame_stride, int32_t count,
                          int32_t width, int32_t height, int32_t stripe_rows, int32_t num_ranks, int32_t rotate_first, void* stream)
{
    if (!d_gathered || !d_imgs || count < 1 || width <= 0 || height <= 0 || stripe_rows <= 0 || num_ranks <= 0 ||
        local_pitch < (size_t)width * 3 || pitch < (size_t)width * 3) return RT_E_INVALID;
    const size_t row_bytes = (size_t)width * 3;
    const bool vec = ((uintptr_t)d_gathered | (uintptr_t)d_imgs | local_pitch | rank_stride | src_frame_stride | pitch | dst_frame_stride | row_bytes) % 16 == 0;
    const size_t row_units = vec ? row_bytes / 16 : row_bytes;
    dim3 grid((unsigned)((row_units * (size_t)height + 255) / 256), 1, (unsigned)count), block(256);
    if (vec)
        hipLaunchKernelGGL(unstripe_kernel<uint4>, grid, block, 0, (hipStream_t)stream, d_gathered, local_pitch, rank_stride, src_frame_stride,
                           d_imgs, pitch, dst_frame_stride, (int)row_units, height, stripe_rows, num_ranks, rotate_first);
    else
        hipLaunchKernelGGL(unstripe_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, d_gathered, local_pitch, rank_stride, src_frame_stride,
                           d_imgs, pitch, dst_frame_stride, (int)row_units, height, stripe_rows, num_ranks, rotate_first);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_unstripe_batch(const uint8_t* d_gathered, size_t local_pitch, size_t rank_stride, size_t src_frame_stride,
                      uint8_t* d_imgs, size_t pitch, size_t dst_frame_stride, int32_t count,
                      int32_t width, int32_t height, int32_t stripe_rows, int32_t num_ranks, void* stream)
{
    return unstripe_batch(d_gathered, local_pitch, rank_stride, src_frame_stride, d_imgs, pitch, dst_frame_stride, count, width, height,
                          stripe_rows, num_ranks, -1, stream);
}

int rt_unstripe_batch_rotating(const uint8_t* d_gathered, size_t local_pitch, size_t rank_stride, size_t src_frame_stride,
                               uint8_t* d_imgs, size_t pitch, size_t dst_frame_stride, int32_t count,
                               int32_t width, int32_t height, int32_t stripe_rows, int32_t num_ranks, int32_t first_frame, void* stream)
{
    if (first_frame < 0) return RT_E_INVALID;
    return unstripe_batch(d_gathered, local_pitch, rank_stride, src_frame_stride, d_imgs, pitch, dst_frame_stride, count, width, height,
                          stripe_rows, num_ranks, first_frame, stream);
}

int rt_unstripe(const uint8_t* d_gathered, size_t local_pitch, size_t rank_stride, uint8_t* d_img, size_t pitch,
                int32_t width, int32_t height, int32_t stripe_rows, int32_t num_ranks, void* stream)
{
    return rt_unstripe_batch(d_gathered, local_pitch, rank_stride, 0, d_img, pitch, 0, 1, width, height, stripe_rows, num_ranks, stream);
}

// ---- queries: what their entry points share --------------------------------------------------------------------------------------
extern "C++" {
namespace {
// the launch shape of a query kernel: one thread per query in workgroups of `block`, and the bytes of a workgroup's LDS stack block
// (spare_rows: the optimistic stack's row, see StackT)
struct QueryShape {
    dim3 groups;
    size_t lds;
};
QueryShape query_shape(int32_t n, int block, int stack_depth, int spare_rows = 0)
{
    return {dim3((unsigned)(((int64_t)n + block - 1) / block)), (size_t)(lds_rows(stack_depth) + spare_rows) * block * sizeof(int)};
}

// a query's params struct, zeroed, with the fields every one of them reads the scene through
template <class P>
P scene_params(const RtScene* s)
{
    P p;
    memset(&p, 0, sizeof p);
    p.records = s->d_records; p.leaf_count = s->d_leaf_count; p.mesh_flags = s->d_mesh_flags; p.instances = s->d_instances;
    p.num_instances = (int32_t)s->instances.size();
    p.stack_depth = s->max_stack;
    return p;
}

// The part of a query call that touches the scene, after the argument checks and the n == 0 return (which take no lock): `launch`
// enqueues on `stream` under the scene's call lock and returns RT_OK or the call's error; the lock is left BEFORE the stream is
// waited for, so a synchronous call does not keep other threads' launches out while its own work runs.
template <class F>
int scene_launch(RtScene* s, void* stream, int synchronize, F&& launch)
{
    {
        RT_SCENE_CALL(s);
        const int rc = launch((hipStream_t)stream);
        if (rc != RT_OK) return rc;
        RT_HIP(hipGetLastError());
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}
}  // namespace
}  // extern "C++"

// ---- ray queries ------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t kQueryBinsBytes = 256;                          // the workspace's counters (16 ints), then the permutation

int launch_query(RtScene* s, QueryParams& q, bool anyhit, void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    if (!s || q.n < 0 || (q.n > 0 && (!q.org || !q.dir))) return RT_E_INVALID;
    if (d_workspace && workspace_bytes < rt_trace_workspace_bytes(q.n)) return RT_E_INVALID;
    if (q.n == 0) return RT_OK;                                  // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        RenderParams p;
        memset(&p, 0, sizeof p);
        fill_scene(p, s);
        p.num_frames = 1;
        if (d_workspace) {
            q.bins = (int32_t*)d_workspace;
            int32_t* order = (int32_t*)((char*)d_workspace + kQueryBinsBytes);
            const unsigned chunks = (unsigned)(((int64_t)q.n + kBinChunk - 1) / kBinChunk);
            RT_HIP(hipMemsetAsync(q.bins, 0, 16 * sizeof(int32_t), st));
            hipLaunchKernelGGL(bin_count_kernel, dim3(chunks), dim3(kBinBlock), 0, st, q);
            hipLaunchKernelGGL(bin_scatter_kernel, dim3(chunks), dim3(kBinBlock), 0, st, q, order);
            q.order = order;
        }
        const QueryShape k = query_shape(q.n, kQueryBlock, p.stack_depth, 1);     // (+ the optimistic stack's spare row)
        if (anyhit) hipLaunchKernelGGL(query_kernel<true>, k.groups, dim3(kQueryBlock), k.lds, st, p, q);
        else hipLaunchKernelGGL(query_kernel<false>, k.groups, dim3(kQueryBlock), k.lds, st, p, q);
        return RT_OK;
    });
}
}  // namespace

size_t rt_trace_workspace_bytes(int32_t n)
{
    return n < 0 ? 0 : kQueryBinsBytes + (size_t)n * sizeof(int32_t);
}

int rt_trace_rays(RtScene* s, const float* d_origins, const float* d_directions, int32_t n, const RtRayHits* out,
                  void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    if (!out) return RT_E_INVALID;
    QueryParams q;
    memset(&q, 0, sizeof q);
    q.org = d_origins; q.dir = d_directions; q.n = n;
    q.t = out->t; q.instance = out->instance; q.triangle = out->triangle;
    q.location = out->location; q.normal = out->normal; q.uv = out->uv; q.pops = out->pops;
    return launch_query(s, q, false, d_workspace, workspace_bytes, stream, synchronize);
}

int rt_occluded(RtScene* s, const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, uint8_t* d_occluded,
                void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    if (n > 0 && !d_occluded) return RT_E_INVALID;
    QueryParams q;
    memset(&q, 0, sizeof q);
    q.org = d_origins; q.dir = d_directions; q.tmax = d_tmax; q.n = n; q.occluded = d_occluded;
    return launch_query(s, q, true, d_workspace, workspace_bytes, stream, synchronize);
}

// ---- visibility masks -------------------------------------------------------------------------------------------------------
int rt_visibility(RtScene* s, const int32_t* d_instance, const float* d_location, const float* d_normal, int32_t width, int32_t height,
                  int32_t count, const float* d_points, int32_t num_points, float bias, const RtVisibility* out, void* stream,
                  int synchronize)
{
    if (!s || !d_instance || !d_location || !d_points || !out) return RT_E_INVALID;
    if ((!out->visible && !out->facing) || (out->facing && !d_normal)) return RT_E_INVALID;
    if (width < 1 || height < 1 || count < 1 || (int64_t)width * height > (int64_t)INT32_MAX / count) return RT_E_INVALID;
    if (num_points < 1 || num_points > 32 || !(bias >= 0.0f && bias < 1.0f)) return RT_E_INVALID;      // (a NaN fails both)
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        RenderParams p;
        memset(&p, 0, sizeof p);
        fill_scene(p, s);
        p.num_frames = 1;
        VisParams v;
        memset(&v, 0, sizeof v);
        v.instance = d_instance; v.location = d_location; v.normal = out->facing ? d_normal : nullptr; v.points = d_points;
        v.width = width; v.height = height; v.num_points = num_points; v.bias = bias;
        v.visible = out->visible; v.facing = out->facing;
        const int tiles_x = (width + kPrimTile - 1) / kPrimTile, tiles_y = (height + kPrimTile - 1) / kPrimTile;
        const size_t lds = query_shape(kQueryBlock, kQueryBlock, p.stack_depth, 1).lds;     // (+ the optimistic stack's spare row)
        // a grid's y and z end at 65 535: as many launches as the tile rows and the frames need
        for (int f0 = 0; f0 < count; f0 += 65535)
            for (int y0 = 0; y0 < tiles_y; y0 += 65535) {
                v.frame0 = f0; v.ty0 = y0;
                const dim3 groups((unsigned)tiles_x, (unsigned)std::min(tiles_y - y0, 65535), (unsigned)std::min(count - f0, 65535));
                hipLaunchKernelGGL(visibility_kernel, groups, dim3(kQueryBlock), lds, st, p, v);
            }
        return RT_OK;
    });
}

// ---- point queries ----------------------------------------------------------------------------------------------------------
int rt_closest_points(RtScene* s, const float* d_points, const float* d_max_distance, int32_t n, const RtPointHits* out, void* stream,
                      int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_points || !out))) return RT_E_INVALID;
    if (n > 0 && !(out->distance || out->instance || out->triangle || out->point || out->normal || out->barycentric || out->uv || out->pops))
        return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        PointParams p = scene_params<PointParams>(s);
        p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
        p.pts = d_points; p.max_distance = d_max_distance; p.n = n;
        p.distance = out->distance; p.instance = out->instance; p.triangle = out->triangle;
        p.point = out->point; p.normal = out->normal; p.barycentric = out->barycentric; p.uv = out->uv; p.pops = out->pops;
        const QueryShape k = query_shape(n, kPointBlock, p.stack_depth);
        hipLaunchKernelGGL(closest_point_kernel, k.groups, dim3(kPointBlock), k.lds, st, p);
        return RT_OK;
    });
}

// ---- segment queries --------------------------------------------------------------------------------------------------------
int rt_closest_to_segments(RtScene* s, const float* d_segments, const float* d_max_distance, int32_t n, const RtSegmentHits* out,
                           void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_segments || !out))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    // what only a full distance traversal gives; what the distance half feeds at all; what the crossing half feeds
    const bool full = out->distance || out->instance || out->triangle || out->parameter || out->segment_point || out->point ||
                      out->normal || out->barycentric || out->uv || out->clearance;
    const bool near = full || out->within || out->pops, cross = out->crossings || out->clearance || out->within;
    if (!near && !cross) return RT_E_INVALID;
    // (both launches under one hold of the scene's lock: no other thread's update comes between the distance and the crossings)
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        SegParams p = scene_params<SegParams>(s);
        p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
        p.segs = d_segments; p.max_distance = d_max_distance; p.n = n;
        p.distance = out->distance; p.instance = out->instance; p.triangle = out->triangle; p.parameter = out->parameter;
        p.segment_point = out->segment_point; p.point = out->point; p.normal = out->normal; p.barycentric = out->barycentric;
        p.uv = out->uv; p.crossings = out->crossings; p.clearance = out->clearance; p.within = out->within; p.pops = out->pops;
        const QueryShape k = query_shape(n, kPointBlock, p.stack_depth);
        if (near && full) hipLaunchKernelGGL(segment_closest_kernel<false>, k.groups, dim3(kPointBlock), k.lds, st, p);
        else if (near) hipLaunchKernelGGL(segment_closest_kernel<true>, k.groups, dim3(kPointBlock), k.lds, st, p);
        if (cross) {
            const QueryShape c = query_shape(n, kCrossBlock, p.stack_depth);
            hipLaunchKernelGGL(segment_crossing_kernel, c.groups, dim3(kCrossBlock), c.lds, st, p);
        }
        return RT_OK;
    });
}

// ---- sphere sweeps ----------------------------------------------------------------------------------------------------------
int rt_sweep_spheres(RtScene* s, const float* d_segments, const float* d_radius, int32_t n, const RtSweepHits* out, void* stream,
                     int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_segments || !d_radius || !out))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    // what only the full traversal gives; hit and pops alone end at the first valid candidate
    const bool full = out->time || out->distance || out->instance || out->triangle || out->centre || out->point || out->normal ||
                      out->contact_normal || out->barycentric || out->uv;
    if (!full && !out->hit && !out->pops) return RT_E_INVALID;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        SweepParams p = scene_params<SweepParams>(s);
        p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
        p.segs = d_segments; p.radius = d_radius; p.n = n;
        p.time = out->time; p.distance = out->distance; p.instance = out->instance; p.triangle = out->triangle; p.centre = out->centre;
        p.point = out->point; p.normal = out->normal; p.contact_normal = out->contact_normal; p.barycentric = out->barycentric;
        p.uv = out->uv; p.hit = out->hit; p.pops = out->pops;
        const QueryShape k = query_shape(n, kPointBlock, p.stack_depth);
        if (full) hipLaunchKernelGGL(sweep_kernel<false>, k.groups, dim3(kPointBlock), k.lds, st, p);
        else hipLaunchKernelGGL(sweep_kernel<true>, k.groups, dim3(kPointBlock), k.lds, st, p);
        return RT_OK;
    });
}

// ---- crossings --------------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
template <bool POINT>
void launch_crossings(const CrossParams& p, hipStream_t st)
{
    const QueryShape k = query_shape(p.n, kCrossBlock, p.stack_depth);
    hipLaunchKernelGGL(crossing_kernel<POINT>, k.groups, dim3(kCrossBlock), k.lds, st, p);
}
}  // namespace
}  // extern "C++"

int rt_count_crossings(RtScene* s, const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n,
                       const RtCrossings* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_origins || !d_directions || !out))) return RT_E_INVALID;
    if (n > 0 && !(out->count || out->winding || out->pops)) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        CrossParams p = scene_params<CrossParams>(s);
        p.org = d_origins; p.dir = d_directions; p.tmax = d_tmax; p.n = n;
        p.count = out->count; p.winding = out->winding; p.pops = out->pops;
        launch_crossings<false>(p, st);
        return RT_OK;
    });
}

int rt_winding_numbers(RtScene* s, const float* d_points, int32_t n, int32_t* d_winding, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_points || !d_winding))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        CrossParams p = scene_params<CrossParams>(s);
        p.org = d_points; p.n = n; p.winding = d_winding;
        launch_crossings<true>(p, st);
        return RT_OK;
    });
}

int rt_signed_distance(RtScene* s, const float* d_points, const float* d_max_distance, int32_t n, float* d_sdf, int32_t* d_winding,
                       void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_points || !d_sdf))) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    // (both launches under one hold of the scene's lock: no other thread's update comes between the distance and its sign)
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        RtPointHits hits;
        memset(&hits, 0, sizeof hits);
        hits.distance = d_sdf;                                   // the distance first, then negated in place where inside
        const int rc = rt_closest_points(s, d_points, d_max_distance, n, &hits, stream, 0);
        if (rc != RT_OK) return rc;
        CrossParams p = scene_params<CrossParams>(s);
        p.org = d_points; p.n = n; p.winding = d_winding; p.sdf = d_sdf;
        launch_crossings<true>(p, st);
        return RT_OK;
    });
}

// ---- list queries: CSR offsets from a family's counts ----------------------------------------------------------------------
extern "C++" {
namespace {
// The *_offsets workspace: the counts (int32 [n]), then the block totals of each level of the scan over n + 1 elements
constexpr size_t kScanAlign = 256;
size_t scan_align(size_t b) { return (b + kScanAlign - 1) / kScanAlign * kScanAlign; }
size_t offsets_bytes(int64_t n, int64_t* level_blocks, int* levels)
{
    size_t bytes = scan_align((size_t)n * sizeof(int32_t));
    int64_t m = n + 1;
    int l = 0;
    for (;;) {
        const int64_t b = (m + kScanBlock - 1) / kScanBlock;
        if (level_blocks) level_blocks[l] = b;
        bytes += scan_align((size_t)b * sizeof(int64_t));
        l++;
        if (b == 1) break;
        m = b;
    }
    if (levels) *levels = l;
    return bytes;
}
size_t offsets_workspace_bytes(int32_t n) { return n > 0 ? offsets_bytes(n, nullptr, nullptr) : 0; }
// the exclusive int64 scan of the counts at the workspace's start (int32 [n]) into d_offsets[0..n], the block totals of each level in
// the rest of the workspace (offsets_bytes' layout): level 0 scans the counts, level l > 0 level l - 1's block totals in
// place, then each block of level l - 1 adds its scanned total on the way down
void scan_offsets(void* d_workspace, int32_t n, int64_t* d_offsets, const int64_t* blocks, int levels, hipStream_t st)
{
    const int32_t* counts = (const int32_t*)d_workspace;
    int64_t* sums[8];
    char* at = (char*)d_workspace + scan_align((size_t)n * sizeof(int32_t));
    for (int l = 0; l < levels; l++) { sums[l] = (int64_t*)at; at += scan_align((size_t)blocks[l] * sizeof(int64_t)); }
    hipLaunchKernelGGL(scan_block_kernel<int32_t>, dim3((unsigned)blocks[0]), dim3(kScanThreads), 0, st, counts, (int64_t)n, d_offsets,
                       (int64_t)n + 1, sums[0]);
    for (int l = 1; l < levels; l++)
        hipLaunchKernelGGL(scan_block_kernel<int64_t>, dim3((unsigned)blocks[l]), dim3(kScanThreads), 0, st, sums[l - 1], blocks[l - 1],
                           sums[l - 1], blocks[l - 1], sums[l]);
    for (int l = levels - 1; l >= 1; l--)
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)blocks[l - 1]), dim3(kScanThreads), 0, st, l >= 2 ? sums[l - 2] : d_offsets,
                           l >= 2 ? blocks[l - 2] : (int64_t)n + 1, sums[l - 1]);
}
// The *_offsets call of a list query, once its own pointers are checked and n > 0: `launch_counts(counts, stream)` runs the family's
// count kernel into the workspace's start, the scan turns the counts into d_offsets[0..n].
template <class F>
int query_offsets(RtScene* s, int32_t n, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* stream, int synchronize,
                  F&& launch_counts)
{
    int64_t blocks[8];
    int levels = 0;
    if (workspace_bytes < offsets_bytes(n, blocks, &levels)) return RT_E_INVALID;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        launch_counts((int32_t*)d_workspace, st);
        scan_offsets(d_workspace, n, d_offsets, blocks, levels, st);
        return RT_OK;
    });
}
}  // namespace
}  // extern "C++"

size_t rt_crossing_offsets_workspace_bytes(int32_t n) { return offsets_workspace_bytes(n); }

int rt_crossing_offsets(RtScene* s, const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, int64_t* d_offsets,
                        void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_origins || !d_directions || !d_offsets || !d_workspace))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched, d_offsets not written
    return query_offsets(s, n, d_offsets, d_workspace, workspace_bytes, stream, synchronize, [&](int32_t* counts, hipStream_t st) {
        CrossParams p = scene_params<CrossParams>(s);
        p.org = d_origins; p.dir = d_directions; p.tmax = d_tmax; p.n = n; p.count = counts;
        launch_crossings<false>(p, st);
    });
}

int rt_list_crossings(RtScene* s, const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, const int64_t* d_offsets,
                      int32_t max_hits, const RtCrossingList* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_origins || !d_directions || !out))) return RT_E_INVALID;
    if ((d_offsets != nullptr) == (max_hits >= 1)) return RT_E_INVALID;     // exactly one of CSR and fixed rooms
    if (n > 0 && !(out->t || out->instance || out->triangle || out->sign || out->barycentric || out->uv || out->point || out->count))
        return RT_E_INVALID;
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        CrossListParams p = scene_params<CrossListParams>(s);
        p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
        p.org = d_origins; p.dir = d_directions; p.tmax = d_tmax; p.n = n;
        p.offsets = d_offsets; p.max_hits = d_offsets ? 0 : max_hits;
        p.t = out->t; p.instance = out->instance; p.triangle = out->triangle; p.sign = out->sign;
        p.barycentric = out->barycentric; p.uv = out->uv; p.point = out->point; p.count = out->count;
        const QueryShape k = query_shape(n, kCrossBlock, p.stack_depth);
        if (p.t && p.instance && p.triangle)                    // the room holds the keys: insertion
            hipLaunchKernelGGL(crossing_list_kernel<false>, k.groups, dim3(kCrossBlock), k.lds, st, p);
        else
            hipLaunchKernelGGL(crossing_list_kernel<true>, k.groups, dim3(kCrossBlock), k.lds, st, p);
        return RT_OK;
    });
}

// ---- nearby triangles -------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
NearbyParams nearby_params(const RtScene* s, const float* d_points, const float* d_max_distance, int32_t n)
{
    NearbyParams p = scene_params<NearbyParams>(s);
    p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
    p.pts = d_points; p.max_distance = d_max_distance; p.n = n;
    return p;
}
}  // namespace
}  // extern "C++"

size_t rt_nearby_offsets_workspace_bytes(int32_t n) { return offsets_workspace_bytes(n); }

int rt_nearby_offsets(RtScene* s, const float* d_points, const float* d_max_distance, int32_t n, int64_t* d_offsets, void* d_workspace,
                      size_t workspace_bytes, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_points || !d_offsets || !d_workspace))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched, d_offsets not written
    return query_offsets(s, n, d_offsets, d_workspace, workspace_bytes, stream, synchronize, [&](int32_t* counts, hipStream_t st) {
        NearbyParams p = nearby_params(s, d_points, d_max_distance, n);
        p.count = counts;
        const QueryShape k = query_shape(n, kPointBlock, p.stack_depth);
        hipLaunchKernelGGL(nearby_count_kernel, k.groups, dim3(kPointBlock), k.lds, st, p);
    });
}

int rt_list_nearby(RtScene* s, const float* d_points, const float* d_max_distance, int32_t n, const int64_t* d_offsets, int32_t max_hits,
                   const RtNearbyList* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_points || !out))) return RT_E_INVALID;
    if ((d_offsets != nullptr) == (max_hits >= 1)) return RT_E_INVALID;     // exactly one of CSR and fixed rooms
    if (n > 0 && !(out->distance && out->instance && out->triangle)) return RT_E_INVALID;     // the room holds the keys
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        NearbyParams p = nearby_params(s, d_points, d_max_distance, n);
        p.offsets = d_offsets; p.max_hits = d_offsets ? 0 : max_hits;
        p.distance = out->distance; p.instance = out->instance; p.triangle = out->triangle;
        p.point = out->point; p.normal = out->normal; p.barycentric = out->barycentric; p.uv = out->uv;
        p.count = out->count; p.pops = out->pops;
        const QueryShape k = query_shape(n, kPointBlock, p.stack_depth);
        hipLaunchKernelGGL(nearby_list_kernel, k.groups, dim3(kPointBlock), k.lds, st, p);
        return RT_OK;
    });
}

// ---- intersecting triangles -------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
TriParams intersect_params(const RtScene* s, const float* d_triangles, const int32_t* d_skip_instance, int32_t n)
{
    TriParams p = scene_params<TriParams>(s);
    p.tri_id = s->d_tri_id;
    p.tris = d_triangles; p.skip = d_skip_instance; p.n = n;
    return p;
}
void launch_intersect_count(const TriParams& p, bool any_only, hipStream_t st)
{
    const QueryShape k = query_shape(p.n, kTriBlock, p.stack_depth);
    if (any_only)
        hipLaunchKernelGGL(intersect_count_kernel<true>, k.groups, dim3(kTriBlock), k.lds, st, p);
    else
        hipLaunchKernelGGL(intersect_count_kernel<false>, k.groups, dim3(kTriBlock), k.lds, st, p);
}
}  // namespace
}  // extern "C++"

int rt_count_intersecting(RtScene* s, const float* d_triangles, const int32_t* d_skip_instance, int32_t n, const RtIntersectCounts* out,
                          void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_triangles || !out))) return RT_E_INVALID;
    if (n > 0 && !(out->count || out->any || out->pops)) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        TriParams p = intersect_params(s, d_triangles, d_skip_instance, n);
        p.count = out->count; p.any = out->any; p.pops = out->pops;
        launch_intersect_count(p, p.any && !p.count, st);       // (any without count: stop at the first pair)
        return RT_OK;
    });
}

size_t rt_intersecting_offsets_workspace_bytes(int32_t n) { return offsets_workspace_bytes(n); }

int rt_intersecting_offsets(RtScene* s, const float* d_triangles, const int32_t* d_skip_instance, int32_t n, int64_t* d_offsets,
                            void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_triangles || !d_offsets || !d_workspace))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched, d_offsets not written
    return query_offsets(s, n, d_offsets, d_workspace, workspace_bytes, stream, synchronize, [&](int32_t* counts, hipStream_t st) {
        TriParams p = intersect_params(s, d_triangles, d_skip_instance, n);
        p.count = counts;
        launch_intersect_count(p, false, st);
    });
}

int rt_list_intersecting(RtScene* s, const float* d_triangles, const int32_t* d_skip_instance, int32_t n, const int64_t* d_offsets,
                         int32_t max_hits, const RtIntersectList* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_triangles || !out))) return RT_E_INVALID;
    if ((d_offsets != nullptr) == (max_hits >= 1)) return RT_E_INVALID;     // exactly one of CSR and fixed rooms
    if (n > 0 && !(out->instance && out->triangle)) return RT_E_INVALID;     // the room holds the keys
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        TriParams p = intersect_params(s, d_triangles, d_skip_instance, n);
        p.offsets = d_offsets; p.max_hits = d_offsets ? 0 : max_hits;
        p.instance = out->instance; p.triangle = out->triangle; p.normal = out->normal; p.segment = out->segment;
        p.count = out->count; p.pops = out->pops;
        const QueryShape k = query_shape(n, kTriBlock, p.stack_depth);
        hipLaunchKernelGGL(intersect_list_kernel, k.groups, dim3(kTriBlock), k.lds, st, p);
        return RT_OK;
    });
}

// ---- triangle distance queries (here for intersect_params: the intersection half is the family above) -----------------------
int rt_closest_to_triangles(RtScene* s, const float* d_triangles, const float* d_max_distance, const int32_t* d_skip_instance, int32_t n,
                            const RtTriangleHits* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_triangles || !out))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    // what only a full distance traversal gives; what the distance half feeds at all; what the intersection half feeds
    const bool full = out->distance || out->instance || out->triangle || out->query_barycentric || out->query_point || out->point ||
                      out->normal || out->barycentric || out->uv || out->clearance;
    const bool near = full || out->within || out->pops, meet = out->intersections || out->clearance || out->within;
    if (!near && !meet) return RT_E_INVALID;
    // (both launches under one hold of the scene's lock: no other thread's update comes between the distance and the intersections)
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        if (near) {
            TdParams p = scene_params<TdParams>(s);
            p.tri_uv = s->d_tri_uv; p.tri_id = s->d_tri_id;
            p.tris = d_triangles; p.max_distance = d_max_distance; p.skip = d_skip_instance; p.n = n;
            p.distance = out->distance; p.instance = out->instance; p.triangle = out->triangle;
            p.query_barycentric = out->query_barycentric; p.query_point = out->query_point; p.point = out->point; p.normal = out->normal;
            p.barycentric = out->barycentric; p.uv = out->uv; p.clearance = out->clearance; p.within = out->within; p.pops = out->pops;
            const QueryShape k = query_shape(n, kPointBlock, p.stack_depth);
            if (full) hipLaunchKernelGGL(triangle_closest_kernel<false>, k.groups, dim3(kPointBlock), k.lds, st, p);
            else hipLaunchKernelGGL(triangle_closest_kernel<true>, k.groups, dim3(kPointBlock), k.lds, st, p);
        }
        if (meet) {
            const TriParams t = intersect_params(s, d_triangles, d_skip_instance, n);
            const QueryShape k = query_shape(n, kTriBlock, t.stack_depth);
            if (out->intersections)
                hipLaunchKernelGGL(triangle_intersect_patch_kernel<true>, k.groups, dim3(kTriBlock), k.lds, st, t, out->intersections,
                                   out->clearance, out->within);
            else
                hipLaunchKernelGGL(triangle_intersect_patch_kernel<false>, k.groups, dim3(kTriBlock), k.lds, st, t, (int32_t*)nullptr,
                                   out->clearance, out->within);
        }
        return RT_OK;
    });
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
BoxParams box_params(const RtScene* s, const float* d_boxes, int32_t n)
{
    BoxParams p = scene_params<BoxParams>(s);
    p.tri_id = s->d_tri_id;
    p.boxes = d_boxes; p.n = n;
    return p;
}
void launch_box_count(const BoxParams& p, bool any_only, hipStream_t st)
{
    const QueryShape k = query_shape(p.n, kTriBlock, p.stack_depth);
    if (any_only)
        hipLaunchKernelGGL(box_count_kernel<true>, k.groups, dim3(kTriBlock), k.lds, st, p);
    else
        hipLaunchKernelGGL(box_count_kernel<false>, k.groups, dim3(kTriBlock), k.lds, st, p);
}
}  // namespace
}  // extern "C++"

int rt_count_in_boxes(RtScene* s, const float* d_boxes, int32_t n, const RtBoxCounts* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_boxes || !out))) return RT_E_INVALID;
    if (n > 0 && !(out->count || out->any || out->pops)) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        BoxParams p = box_params(s, d_boxes, n);
        p.count = out->count; p.any = out->any; p.pops = out->pops;
        launch_box_count(p, p.any && !p.count, st);             // (any without count: stop at the first pair)
        return RT_OK;
    });
}

size_t rt_box_offsets_workspace_bytes(int32_t n) { return offsets_workspace_bytes(n); }

int rt_box_offsets(RtScene* s, const float* d_boxes, int32_t n, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes,
                   void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_boxes || !d_offsets || !d_workspace))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched, d_offsets not written
    return query_offsets(s, n, d_offsets, d_workspace, workspace_bytes, stream, synchronize, [&](int32_t* counts, hipStream_t st) {
        BoxParams p = box_params(s, d_boxes, n);
        p.count = counts;
        launch_box_count(p, false, st);
    });
}

int rt_list_in_boxes(RtScene* s, const float* d_boxes, int32_t n, const int64_t* d_offsets, int32_t max_hits, const RtBoxList* out,
                     void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_boxes || !out))) return RT_E_INVALID;
    if ((d_offsets != nullptr) == (max_hits >= 1)) return RT_E_INVALID;     // exactly one of CSR and fixed rooms
    if (n > 0 && !(out->instance && out->triangle)) return RT_E_INVALID;     // the room holds the keys
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        BoxParams p = box_params(s, d_boxes, n);
        p.offsets = d_offsets; p.max_hits = d_offsets ? 0 : max_hits;
        p.instance = out->instance; p.triangle = out->triangle;
        p.count = out->count; p.pops = out->pops;
        const QueryShape k = query_shape(n, kTriBlock, p.stack_depth);
        hipLaunchKernelGGL(box_list_kernel, k.groups, dim3(kTriBlock), k.lds, st, p);
        return RT_OK;
    });
}

int rt_occupancy_grid(RtScene* s, const float* origin, const float* spacing, const int32_t* dims, uint8_t* d_occupied, int32_t* d_count,
                      void* stream, int synchronize)
{
    if (!s || !origin || !spacing || !dims) return RT_E_INVALID;
    for (int a = 0; a < 3; a++)
        if (dims[a] < 0 || dims[a] > (1 << 24)) return RT_E_INVALID;        // ((float)i is exact up to 2^24)
    int64_t cells = (int64_t)dims[0] * dims[1], bricks = 1;      // (<= 2^48)
    if (cells > (int64_t)INT32_MAX && dims[2] > 0) return RT_E_INVALID;
    cells = dims[2] > 0 ? cells * dims[2] : 0;                   // (<= 2^55)
    if (cells > (int64_t)INT32_MAX) return RT_E_INVALID;
    for (int a = 0; a < 3; a++) bricks *= (dims[a] + 3) / 4;
    if (cells > 0 && !(d_occupied || d_count)) return RT_E_INVALID;
    if (cells == 0) return RT_OK;                                // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        BoxParams p = box_params(s, nullptr, (int32_t)cells);
        for (int a = 0; a < 3; a++) {
            p.origin[a] = origin[a]; p.spacing[a] = spacing[a]; p.dims[a] = dims[a];
            p.bricks[a] = (uint32_t)((dims[a] + 3) / 4);
        }
        p.count = d_count; p.any = d_occupied;
        const dim3 groups((unsigned)(bricks < 65536 ? bricks : 65536), (unsigned)((bricks + 65535) / 65536));    // (bricks <= cells)
        const size_t lds = query_shape(1, kTriBlock, p.stack_depth).lds;
        if (p.any && !p.count)                                   // (occupied without count: stop at the first pair)
            hipLaunchKernelGGL(box_grid_kernel<true>, groups, dim3(kTriBlock), lds, st, p);
        else
            hipLaunchKernelGGL(box_grid_kernel<false>, groups, dim3(kTriBlock), lds, st, p);
        return RT_OK;
    });
}

// ---- plane sections ---------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
SecParams section_params(const RtScene* s, const float* d_planes, int32_t n)
{
    SecParams p = scene_params<SecParams>(s);
    p.tri_id = s->d_tri_id;
    p.planes = d_planes; p.n = n;
    return p;
}
void launch_section_count(const SecParams& p, bool any_only, hipStream_t st)
{
    const QueryShape k = query_shape(p.n, kTriBlock, p.stack_depth);
    if (any_only)
        hipLaunchKernelGGL(section_count_kernel<true>, k.groups, dim3(kTriBlock), k.lds, st, p);
    else
        hipLaunchKernelGGL(section_count_kernel<false>, k.groups, dim3(kTriBlock), k.lds, st, p);
}
}  // namespace
}  // extern "C++"

int rt_count_sections(RtScene* s, const float* d_planes, int32_t n, const RtSectionCounts* out, void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_planes || !out))) return RT_E_INVALID;
    if (n > 0 && !(out->count || out->any || out->pops)) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        SecParams p = section_params(s, d_planes, n);
        p.count = out->count; p.any = out->any; p.pops = out->pops;
        launch_section_count(p, p.any && !p.count, st);         // (any without count: stop at the first pair)
        return RT_OK;
    });
}

size_t rt_section_offsets_workspace_bytes(int32_t n) { return offsets_workspace_bytes(n); }

int rt_section_offsets(RtScene* s, const float* d_planes, int32_t n, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes,
                       void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_planes || !d_offsets || !d_workspace))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched, d_offsets not written
    return query_offsets(s, n, d_offsets, d_workspace, workspace_bytes, stream, synchronize, [&](int32_t* counts, hipStream_t st) {
        SecParams p = section_params(s, d_planes, n);
        p.count = counts;
        launch_section_count(p, false, st);
    });
}

int rt_list_sections(RtScene* s, const float* d_planes, int32_t n, const int64_t* d_offsets, int32_t max_hits, const RtSectionList* out,
                     void* stream, int synchronize)
{
    if (!s || n < 0 || (n > 0 && (!d_planes || !out))) return RT_E_INVALID;
    if ((d_offsets != nullptr) == (max_hits >= 1)) return RT_E_INVALID;     // exactly one of CSR and fixed rooms
    if (n > 0 && !(out->instance && out->triangle)) return RT_E_INVALID;     // the room holds the keys
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        SecParams p = section_params(s, d_planes, n);
        p.offsets = d_offsets; p.max_hits = d_offsets ? 0 : max_hits;
        p.instance = out->instance; p.triangle = out->triangle; p.segment = out->segment; p.normal = out->normal;
        p.count = out->count; p.pops = out->pops;
        const QueryShape k = query_shape(n, kTriBlock, p.stack_depth);
        hipLaunchKernelGGL(section_list_kernel, k.groups, dim3(kTriBlock), k.lds, st, p);
        return RT_OK;
    });
}

// ---- region queries -----------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
bool region_planes_ok(int32_t planes) { return planes >= 1 && planes <= kRegionMaxPlanes; }
RegParams region_params(const RtScene* s, const float* d_regions, int32_t n, int32_t planes)
{
    RegParams p = scene_params<RegParams>(s);
    p.tri_id = s->d_tri_id;
    p.regions = d_regions; p.n = n; p.planes = planes;
    return p;
}
// the kernel of the smallest plane capacity that holds the call's K
template <int KT>
void launch_region_count_kt(const RegParams& p, bool any_only, const QueryShape& k, hipStream_t st)
{
    if (any_only)
        hipLaunchKernelGGL((region_count_kernel<KT, true>), k.groups, dim3(kTriBlock), k.lds, st, p);
    else
        hipLaunchKernelGGL((region_count_kernel<KT, false>), k.groups, dim3(kTriBlock), k.lds, st, p);
}
void launch_region_count(const RegParams& p, bool any_only, hipStream_t st)
{
    const QueryShape k = query_shape(p.n, kTriBlock, p.stack_depth);
    if (p.planes <= 2) launch_region_count_kt<2>(p, any_only, k, st);
    else if (p.planes <= 4) launch_region_count_kt<4>(p, any_only, k, st);
    else if (p.planes <= 6) launch_region_count_kt<6>(p, any_only, k, st);
    else launch_region_count_kt<8>(p, any_only, k, st);
}
void launch_region_list(const RegParams& p, hipStream_t st)
{
    const QueryShape k = query_shape(p.n, kTriBlock, p.stack_depth);
    if (p.planes <= 2) hipLaunchKernelGGL(region_list_kernel<2>, k.groups, dim3(kTriBlock), k.lds, st, p);
    else if (p.planes <= 4) hipLaunchKernelGGL(region_list_kernel<4>, k.groups, dim3(kTriBlock), k.lds, st, p);
    else if (p.planes <= 6) hipLaunchKernelGGL(region_list_kernel<6>, k.groups, dim3(kTriBlock), k.lds, st, p);
    else hipLaunchKernelGGL(region_list_kernel<8>, k.groups, dim3(kTriBlock), k.lds, st, p);
}
}  // namespace
}  // extern "C++"

int rt_count_in_regions(RtScene* s, const float* d_regions, int32_t n, int32_t planes_per_region, const RtRegionCounts* out, void* stream,
                        int synchronize)
{
    if (!s || n < 0 || !region_planes_ok(planes_per_region) || (n > 0 && (!d_regions || !out))) return RT_E_INVALID;
    if (n > 0 && !(out->count || out->inside || out->any || out->pops)) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        RegParams p = region_params(s, d_regions, n, planes_per_region);
        p.count = out->count; p.inside = out->inside; p.any = out->any; p.pops = out->pops;
        launch_region_count(p, p.any && !p.count && !p.inside, st);     // (any without count or inside: stop at the first pair)
        return RT_OK;
    });
}

size_t rt_region_offsets_workspace_bytes(int32_t n) { return offsets_workspace_bytes(n); }

int rt_region_offsets(RtScene* s, const float* d_regions, int32_t n, int32_t planes_per_region, int64_t* d_offsets, void* d_workspace,
                      size_t workspace_bytes, void* stream, int synchronize)
{
    if (!s || n < 0 || !region_planes_ok(planes_per_region) || (n > 0 && (!d_regions || !d_offsets || !d_workspace))) return RT_E_INVALID;
    if (n == 0) return RT_OK;                                    // nothing launched, d_offsets not written
    return query_offsets(s, n, d_offsets, d_workspace, workspace_bytes, stream, synchronize, [&](int32_t* counts, hipStream_t st) {
        RegParams p = region_params(s, d_regions, n, planes_per_region);
        p.count = counts;
        launch_region_count(p, false, st);
    });
}

int rt_list_in_regions(RtScene* s, const float* d_regions, int32_t n, int32_t planes_per_region, const int64_t* d_offsets, int32_t max_hits,
                       const RtRegionList* out, void* stream, int synchronize)
{
    if (!s || n < 0 || !region_planes_ok(planes_per_region) || (n > 0 && (!d_regions || !out))) return RT_E_INVALID;
    if ((d_offsets != nullptr) == (max_hits >= 1)) return RT_E_INVALID;     // exactly one of CSR and fixed rooms
    if (n > 0 && !(out->instance && out->triangle)) return RT_E_INVALID;     // the room holds the keys
    if (n == 0) return RT_OK;
    return scene_launch(s, stream, synchronize, [&](hipStream_t st) -> int {
        RegParams p = region_params(s, d_regions, n, planes_per_region);
        p.offsets = d_offsets; p.max_hits = d_offsets ? 0 : max_hits;
        p.instance = out->instance; p.triangle = out->triangle; p.flag = out->inside; p.normal = out->normal;
        p.count = out->count; p.pops = out->pops;
        launch_region_list(p, st);
        return RT_OK;
    });
}

int rt_camera_rays(const RtCameraParams* cam, float* d_origins, float* d_directions, void* stream, int synchronize)
{
    if (!camera_ok(cam) || !d_origins || !d_directions) return RT_E_INVALID;
    FrameParams f;
    memset(&f, 0, sizeof f);
    fill_frame(f, cam);
    const size_t npix = (size_t)cam->width * (size_t)cam->height;
    if ((npix + 255) / 256 > (size_t)INT32_MAX) return RT_E_INVALID;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, cam->width, npix,
                       d_origins, d_directions);
    RT_HIP(hipGetLastError());
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_camera_directions(const RtCameraParams* cam, float* d_dirs, void* stream, int synchronize)
{
    if (!camera_ok(cam) || !d_dirs) return RT_E_INVALID;
    FrameParams f;
    memset(&f, 0, sizeof f);
    fill_frame(f, cam);
    const size_t npix = (size_t)cam->width * (size_t)cam->height;
    if ((npix + 255) / 256 > (size_t)INT32_MAX) return RT_E_INVALID;
    hipLaunchKernelGGL(camera_directions_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, cam->width, npix, d_dirs);
    RT_HIP(hipGetLastError());
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_ray_table_create(const float* d_dirs, int32_t width, int32_t height, void* stream, int synchronize, RtRayTable** out)
{
    if (!d_dirs || !out || width < 1 || height < 1) return RT_E_INVALID;
    const int32_t tiles_x = (width + kPrimTile - 1) / kPrimTile, tiles_y = (height + kPrimTile - 1) / kPrimTile;
    const size_t ntiles = (size_t)tiles_x * (size_t)tiles_y;
    if (tiles_y > 65535 || ntiles > ((size_t)1 << 24)) return RT_E_INVALID;     // (launch_gbuffer's and dir_table_prepare's limits)
    RtRayTable* t = new (std::nothrow) RtRayTable;
    if (!t) return RT_E_NOMEM;
    t->width = width; t->height = height; t->tiles_x = tiles_x; t->tiles_y = tiles_y;
    t->bytes = ntiles * 3 * 64 * sizeof(float);
    t->d_table = nullptr;
    if (hipMalloc((void**)&t->d_table, t->bytes) != hipSuccess) { (void)hipGetLastError(); delete t; return RT_E_NOMEM; }
    const size_t nwords = ntiles * 3 * 64;                      // <= 2^24 * 192: the grid's x holds it
    hipLaunchKernelGGL(ray_table_pack_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)d_dirs,
                       width, height, tiles_x, nwords, (uint32_t*)t->d_table);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && synchronize) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { (void)hipFree(t->d_table); delete t; return (int)e; }
    *out = t;
    return RT_OK;
}

int rt_ray_table_info(const RtRayTable* t, int32_t* width, int32_t* height, size_t* device_bytes)
{
    if (!t) return RT_E_INVALID;
    if (width) *width = t->width;
    if (height) *height = t->height;
    if (device_bytes) *device_bytes = t->bytes;
    return RT_OK;
}

int rt_ray_table_destroy(RtRayTable* t)
{
    if (!t) return RT_OK;
    const hipError_t e = hipFree(t->d_table);
    delete t;
    return e == hipSuccess ? RT_OK : (int)e;
}

int rt_ray_table_rays(const RtRayTable* t, const RtCameraParams* pose, float* d_origins, float* d_directions, void* stream, int synchronize)
{
    if (!t || !camera_ok(pose) || !d_origins || !d_directions) return RT_E_INVALID;
    if (pose->width != t->width || pose->height != t->height) return RT_E_INVALID;
    FrameParams f;
    memset(&f, 0, sizeof f);
    fill_frame(f, pose);                                        // (K_inv and D travel along unread)
    const size_t npix = (size_t)t->width * (size_t)t->height;
    hipLaunchKernelGGL(ray_table_rays_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, t->d_table, t->width,
                       t->tiles_x, npix, d_origins, d_directions);
    RT_HIP(hipGetLastError());
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

// ---- point clouds (include/rt_hip.h "point clouds") ------------------------------------------------------
extern "C++" {
namespace {
// The workspace of one rt_point_cloud_offsets call, every part on a 256-byte boundary: the scan's own block (the chunk counts, int32
// [nchunks], and its levels' block totals: offsets_bytes), the scanned chunk offsets (int64 [nchunks + 1]), the chunks' ballots
// (uint64 [nchunks]), then the staged planes [count][px](xk) the fields need.  Both calls derive it from the same four arguments.
struct CloudLayout {
    int64_t px;
    int32_t chunks_per_frame, nchunks;
    int64_t blocks[8];
    int levels;
    size_t chunk_offsets, keep, t, instance, triangle, location, normal, uv;    // byte offsets; 0 = not staged (the scan's block is first)
    size_t bytes;
};
bool cloud_layout(int32_t width, int32_t height, int32_t count, uint32_t fields, CloudLayout& L)
{
    if (width < 1 || height < 1 || count < 1 || count > kMaxBatch || fields == 0 || (fields & ~RT_CLOUD_ALL)) return false;
    L.px = (int64_t)width * (int64_t)height;
    const int64_t per_frame = (L.px + kCloudChunk - 1) / kCloudChunk, n = per_frame * count;
    if (n > (int64_t)INT32_MAX) return false;                   // (the scan's int32 n)
    L.chunks_per_frame = (int32_t)per_frame; L.nchunks = (int32_t)n;
    size_t at = offsets_bytes(n, L.blocks, &L.levels);
    const size_t pixels = (size_t)L.px * (size_t)count;
    auto part = [&](bool wanted, size_t bytes) { const size_t o = wanted ? at : 0; if (wanted) at += scan_align(bytes); return o; };
    L.chunk_offsets = part(true, ((size_t)n + 1) * sizeof(int64_t));
    L.keep = part(true, (size_t)n * sizeof(unsigned long long));
    L.t = part(true, pixels * sizeof(float));
    L.instance = part(true, pixels * sizeof(int32_t));
    L.triangle = part(fields & RT_CLOUD_TRIANGLE, pixels * sizeof(int32_t));
    L.location = part(fields & (RT_CLOUD_POSITION | RT_CLOUD_LOCAL), pixels * 3 * sizeof(float));
    L.normal = part(fields & RT_CLOUD_NORMAL, pixels * 3 * sizeof(float));
    L.uv = part(fields & RT_CLOUD_UV, pixels * 2 * sizeof(float));
    L.bytes = at;
    return true;
}
// what both calls ask of their frames (render_gbuffer's checks of cams and count)
bool cloud_frames_ok(const RtCameraParams* cams, int32_t count)
{
    if (!cams || count < 1 || count > kMaxBatch || !camera_ok(&cams[0])) return false;
    for (int i = 1; i < count; i++) if (cams[i].width != cams[0].width || cams[i].height != cams[0].height) return false;
    return true;
}
// the part of *_offsets that reads the workspace only: the count kernel over the staged t and instance planes, the scan, the frame offsets
int cloud_count_and_scan(const CloudLayout& L, void* d_workspace, int32_t count, float min_range, float max_range, const uint8_t* d_mask,
                         int64_t* d_offsets, hipStream_t st)
{
    char* const ws = (char*)d_workspace;
    CloudCountParams c;
    c.t = (const float*)(ws + L.t); c.instance = (const int32_t*)(ws + L.instance); c.mask = d_mask;
    c.px = L.px; c.chunks_per_frame = L.chunks_per_frame; c.nchunks = L.nchunks;
    c.min_range = min_range; c.max_range = max_range;
    c.counts = (int32_t*)ws; c.keep = (unsigned long long*)(ws + L.keep);
    const unsigned grid = (unsigned)(((int64_t)L.nchunks + kCloudBlock / kCloudChunk - 1) / (kCloudBlock / kCloudChunk));
    hipLaunchKernelGGL(cloud_count_kernel, dim3(grid), dim3(kCloudBlock), 0, st, c);
    scan_offsets(d_workspace, L.nchunks, (int64_t*)(ws + L.chunk_offsets), L.blocks, L.levels, st);
    hipLaunchKernelGGL(cloud_frame_offsets_kernel, dim3(1), dim3(64), 0, st, (const int64_t*)(ws + L.chunk_offsets), L.chunks_per_frame, count,
                       d_offsets);
    RT_HIP(hipGetLastError());
    return RT_OK;
}
int point_cloud_offsets(RtScene* s, const RtRayTable* table, const RtCameraParams* cams, int32_t count, float min_range, float max_range,
                        const uint8_t* d_mask, uint32_t fields, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* stream,
                        int synchronize)
{
    // (every argument is judged before the scene is touched)
    if (!s || !cloud_frames_ok(cams, count) || !d_offsets || !d_workspace) return RT_E_INVALID;
    if (!(min_range <= max_range)) return RT_E_INVALID;         // (a NaN bound fails the comparison)
    CloudLayout L;
    if (!cloud_layout(cams[0].width, cams[0].height, count, fields, L) || workspace_bytes < L.bytes) return RT_E_INVALID;
    if (table && (cams[0].width != table->width || cams[0].height != table->height)) return RT_E_INVALID;
    char* const ws = (char*)d_workspace;
    const hipStream_t st = (hipStream_t)stream;
    {
        RT_SCENE_CALL(s);
        RenderParams p;
        int rc = fill_params(p, s, cams, nullptr, count, 0, true);
        if (rc) return rc;
        GBufParams g;
        memset(&g, 0, sizeof g);
        g.t = (float*)(ws + L.t); g.instance = (int32_t*)(ws + L.instance);
        if (L.triangle) g.triangle = (int32_t*)(ws + L.triangle);
        if (L.location) g.location = (float*)(ws + L.location);
        if (L.normal) g.normal = (float*)(ws + L.normal);
        if (L.uv) g.uv = (float*)(ws + L.uv);
        if ((rc = launch_gbuffer(s, p, g, st, table ? table->d_table : nullptr))) return rc;
    }
    // (the scene is no longer needed: the rest reads the workspace only)
    if (int rc = cloud_count_and_scan(L, d_workspace, count, min_range, max_range, d_mask, d_offsets, st)) return rc;
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}
// the staging planes g renders for `fields` into a workspace of layout L
void cloud_staging(const CloudLayout& L, char* ws, GBufParams& g)
{
    memset(&g, 0, sizeof g);
    g.t = (float*)(ws + L.t); g.instance = (int32_t*)(ws + L.instance);
    if (L.triangle) g.triangle = (int32_t*)(ws + L.triangle);
    if (L.location) g.location = (float*)(ws + L.location);
    if (L.normal) g.normal = (float*)(ws + L.normal);
    if (L.uv) g.uv = (float*)(ws + L.uv);
}
// rt_point_cloud_offsets_rolling: the staging planes by the rolling launch, the pose records behind the static layout (L.bytes is a
// multiple of 256), then the count, the scan and the frame offsets as they are
int point_cloud_offsets_rolling(RtScene* s, const RtRayTable* table, const RtRollingPose* poses, int32_t count, int32_t axis, int32_t slice_pixels,
                                float min_range, float max_range, const uint8_t* d_mask, uint32_t fields, int64_t* d_offsets, void* d_workspace,
                                size_t workspace_bytes, void* stream, int synchronize)
{
    int32_t slices = 0;
    if (!s || !table || !poses || !d_offsets || !d_workspace || count < 1 || count > kMaxBatch || !rolling_axis_ok(axis, slice_pixels)) return RT_E_INVALID;
    if (!(min_range <= max_range) || fields == 0 || (fields & ~RT_CLOUD_ALL)) return RT_E_INVALID;     // (a NaN bound fails the comparison)
    CloudLayout L;                                              // (the table is looked at last: whatever can be judged without it has been)
    if (!rolling_shape(table->width, table->height, axis, slice_pixels, slices) || !cloud_layout(table->width, table->height, count, fields, L) ||
        workspace_bytes < L.bytes + rolling_record_bytes(count, slices)) return RT_E_INVALID;
    char* const ws = (char*)d_workspace;
    const hipStream_t st = (hipStream_t)stream;
    GBufParams g;
    cloud_staging(L, ws, g);
    int rc = rolling_render(s, table, poses, count, slices, axis, slice_pixels, nullptr, 0, g, nullptr, ws + L.bytes, st);
    if (rc) return rc;
    if ((rc = cloud_count_and_scan(L, d_workspace, count, min_range, max_range, d_mask, d_offsets, st))) return rc;
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}
// what both fills ask of `out`: no pointer whose plane was not staged, something wanted
bool cloud_outputs_ok(const RtPointCloud* out, uint32_t fields)
{
    const void* const wanted[9] = { out->range, out->pixel, out->frame, out->instance, out->triangle, out->position, out->local, out->normal, out->uv };
    bool any = false;
    for (int k = 0; k < 9; k++) {
        if (wanted[k] && !(fields & (1u << k))) return false;   // (its plane was not staged)
        any = any || wanted[k];
    }
    return any;
}
// the fill's parameters but the poses
void cloud_fill_params(const CloudLayout& L, const char* ws, int64_t capacity, const RtPointCloud* out, CloudFillParams& c)
{
    memset(&c, 0, sizeof c);
    c.chunk_offsets = (const int64_t*)(ws + L.chunk_offsets); c.keep = (const unsigned long long*)(ws + L.keep);
    c.t = (const float*)(ws + L.t); c.instance = (const int32_t*)(ws + L.instance);
    if (L.triangle) c.triangle = (const int32_t*)(ws + L.triangle);
    if (L.location) c.location = (const float*)(ws + L.location);
    if (L.normal) c.normal = (const float*)(ws + L.normal);
    if (L.uv) c.uv = (const float*)(ws + L.uv);
    c.px = L.px; c.chunks_per_frame = L.chunks_per_frame; c.nchunks = L.nchunks; c.capacity = capacity;
    c.range = out->range; c.pixel = out->pixel; c.frame = out->frame; c.out_instance = out->instance; c.out_triangle = out->triangle;
    c.position = out->position; c.local = out->local; c.out_normal = out->normal; c.out_uv = out->uv;
}
}  // namespace
}  // extern "C++"

size_t rt_point_cloud_workspace_bytes(int32_t width, int32_t height, int32_t count, uint32_t fields)
{
    CloudLayout L;
    return cloud_layout(width, height, count, fields, L) ? L.bytes : 0;
}

int rt_point_cloud_offsets(RtScene* s, const RtCameraParams* cams, int32_t count, float min_range, float max_range, const uint8_t* d_mask,
                           uint32_t fields, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    return point_cloud_offsets(s, nullptr, cams, count, min_range, max_range, d_mask, fields, d_offsets, d_workspace, workspace_bytes, stream,
                               synchronize);
}

int rt_point_cloud_offsets_table(RtScene* s, const RtRayTable* table, const RtCameraParams* poses, int32_t count, float min_range,
                                 float max_range, const uint8_t* d_mask, uint32_t fields, int64_t* d_offsets, void* d_workspace,
                                 size_t workspace_bytes, void* stream, int synchronize)
{
    if (!table) return RT_E_INVALID;
    return point_cloud_offsets(s, table, poses, count, min_range, max_range, d_mask, fields, d_offsets, d_workspace, workspace_bytes, stream,
                               synchronize);
}

int rt_point_cloud_fill(const RtCameraParams* cams, int32_t count, uint32_t fields, const void* d_workspace, size_t workspace_bytes,
                        int64_t capacity, const RtPointCloud* out, void* stream, int synchronize)
{
    if (!cloud_frames_ok(cams, count) || !d_workspace || !out || capacity < 0) return RT_E_INVALID;
    CloudLayout L;
    if (!cloud_layout(cams[0].width, cams[0].height, count, fields, L) || workspace_bytes < L.bytes) return RT_E_INVALID;
    if (!cloud_outputs_ok(out, fields)) return RT_E_INVALID;
    if (capacity > 0) {
        CloudFillParams c;
        cloud_fill_params(L, (const char*)d_workspace, capacity, out, c);
        for (int i = 0; i < count; i++) {
            c.q_pose[i] = euler2quat(v3(cams[i].camera_pose[3], cams[i].camera_pose[4], cams[i].camera_pose[5]));
            for (int a = 0; a < 3; a++) c.origin[i][a] = cams[i].camera_pose[a];
        }
        const unsigned grid = (unsigned)(((int64_t)L.nchunks + kCloudBlock / kCloudChunk - 1) / (kCloudBlock / kCloudChunk));
        hipLaunchKernelGGL(cloud_fill_kernel, dim3(grid), dim3(kCloudBlock), 0, (hipStream_t)stream, c);
        RT_HIP(hipGetLastError());
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

size_t rt_point_cloud_rolling_workspace_bytes(int32_t width, int32_t height, int32_t count, uint32_t fields, int32_t slices)
{
    CloudLayout L;
    const size_t rec = rolling_record_bytes(count, slices);
    return rec && cloud_layout(width, height, count, fields, L) ? L.bytes + rec : 0;
}

int rt_point_cloud_offsets_rolling(RtScene* s, const RtRayTable* table, const RtRollingPose* poses, int32_t count, int32_t axis,
                                   int32_t slice_pixels, float min_range, float max_range, const uint8_t* d_mask, uint32_t fields,
                                   int64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* stream, int synchronize)
{
    return point_cloud_offsets_rolling(s, table, poses, count, axis, slice_pixels, min_range, max_range, d_mask, fields, d_offsets, d_workspace,
                                       workspace_bytes, stream, synchronize);
}

int rt_point_cloud_fill_rolling(int32_t width, int32_t height, int32_t count, int32_t axis, int32_t slice_pixels, uint32_t fields,
                                const void* d_workspace, size_t workspace_bytes, int64_t capacity, const RtPointCloud* out, void* stream,
                                int synchronize)
{
    int32_t slices = 0;
    if (!d_workspace || !out || capacity < 0 || !rolling_shape(width, height, axis, slice_pixels, slices)) return RT_E_INVALID;
    CloudLayout L;
    if (!cloud_layout(width, height, count, fields, L) || workspace_bytes < L.bytes + rolling_record_bytes(count, slices)) return RT_E_INVALID;
    if (!cloud_outputs_ok(out, fields)) return RT_E_INVALID;
    if (capacity > 0) {
        CloudFillParams c;
        cloud_fill_params(L, (const char*)d_workspace, capacity, out, c);
        CloudRollParams r;
        r.records = (const RollRecord*)((const char*)d_workspace + L.bytes);
        r.width = width; r.slices = slices; r.axis = axis; r.slice_pixels = slice_pixels;
        const unsigned grid = (unsigned)(((int64_t)L.nchunks + kCloudBlock / kCloudChunk - 1) / (kCloudBlock / kCloudChunk));
        hipLaunchKernelGGL(cloud_fill_rolling_kernel, dim3(grid), dim3(kCloudBlock), 0, (hipStream_t)stream, c, r);
        RT_HIP(hipGetLastError());
    }
    RT_WAIT_IF(synchronize, stream);
    return RT_OK;
}

int rt_timer_create(RtTimer** t)
{
    if (!t) return RT_E_INVALID;
    RtTimer* r = new (std::nothrow) RtTimer;
    if (!r) return RT_E_NOMEM;
    hipError_t e = hipEventCreate(&r->start);
    if (e == hipSuccess) e = hipEventCreate(&r->stop);
    if (e != hipSuccess) { delete r; return (int)e; }
    *t = r;
    return RT_OK;
}
int rt_timer_start(RtTimer* t, void* stream) { if (!t) return RT_E_INVALID; RT_HIP(hipEventRecord(t->start, (hipStream_t)stream)); return RT_OK; }
int rt_timer_stop(RtTimer* t, void* stream) { if (!t) return RT_E_INVALID; RT_HIP(hipEventRecord(t->stop, (hipStream_t)stream)); return RT_OK; }
int rt_timer_elapsed_ms(RtTimer* t, float* ms)
{
    if (!t || !ms) return RT_E_INVALID;
    RT_HIP(hipEventSynchronize(t->stop));
    RT_HIP(hipEventElapsedTime(ms, t->start, t->stop));
    return RT_OK;
}
int rt_timer_destroy(RtTimer* t)
{
    if (!t) return RT_OK;
    (void)hipEventDestroy(t->start); (void)hipEventDestroy(t->stop);
    delete t;
    return RT_OK;
}

}  // extern "C"
