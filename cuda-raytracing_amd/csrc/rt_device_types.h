// rt_device_types.h -- device-side scene layout of librt_hip.so (see DESIGN.md "Data layout in HBM").
#pragma once
#include <cstdint>
#include "rt_math.h"

namespace rt {

// Traversal-stack entry / child reference, 32 bits:
//   >= 0                      interior node: index of its record (scene-wide record array)
//   bit 31 set                leaf: bits 0..25 = index of its first triangle record in the same array,
//                             bits 26..30 = triangle count 0..30, or 31 = read leaf_count[slot]
constexpr int32_t kLeafFlag = (int32_t)0x80000000u;
constexpr int kSlotBits = 26;
constexpr int32_t kSlotMask = (1 << kSlotBits) - 1;
constexpr int kMaxStack = 64;
constexpr int32_t kBoxUnordered = 1;    // mesh_flags bit 0: the octant-specialised slab test must not be used on this mesh

// the twelve box words of an interior record: true when both boxes have min <= max on every axis (false for any NaN)
RT_HD bool boxes_ordered(const float* w)
{
    return w[0] <= w[3] && w[1] <= w[4] && w[2] <= w[5] && w[6] <= w[9] && w[7] <= w[10] && w[8] <= w[11];
}

// Interior node: 64 B = 4 x float4, holds BOTH children's boxes so one pop costs one 64-B
// record instead of the reference's three 48-B d_BVHTree loads (raycast.cu:62,69,70).
//   q0 = a.min.x a.min.y a.min.z a.max.x
//   q1 = a.max.y a.max.z b.min.x b.min.y
//   q2 = b.min.z b.max.x b.max.y b.max.z
//   q3 = ref_a   ref_b   (2 spare words)
//
// Triangle record: 64 B = 4 x float4 in leaf ("slot") order, so a leaf is a contiguous range
// and the per-leaf index lists of BVHTree.hpp:97-111 disappear from the traversal.
//   t0 = v0.x v0.y v0.z n.x
//   t1 = n.y  n.z  e0.x e0.y          e0 = v2 - v0, e1 = v1 - v0   (TrianglePrimitive.hpp:154-155)
//   t2 = e0.z e1.x e1.y e1.z
//   t3 = dot00 dot01 dot11 invDenom   (TrianglePrimitive.hpp:158-164: ray-independent, so
//                                      precomputed on the host with the same fp32 operations)

struct DevInstance {            // 144 B
    Q4 q_rot;                   // euler2quat(rotation)          raycast.cu:33
    Q4 q_pose;                  // euler2quat(pose ypr)          raycast.cu:40
    Q4 q_inv_pose;              // euler2quat(inv_pose ypr)      raycast.cu:102
    Q4 q_inv_rot;               // euler2quat(inv_rotation)      raycast.cu:115
    float pose_xyz[3];
    float inv_pose_xyz[3];
    float scale[3];
    float inv_scale[3];
    int32_t root_ref;           // stack entry of the mesh root
    int32_t material_index;
    int32_t mesh_index;
    int32_t exact_uv;           // mesh has uv values that could make uv.x == FLT_MAX (raycast.cu:96)
    int32_t identity_inv;       // scale == 1, inv_pose == 0, q_inv_pose == (1,0,0,0): mesh -> world is the identity
    int32_t unit_inv;           // scale == 1, q_inv_pose == (1,0,0,0): mesh -> world is a translation (or the identity)
    int32_t pad_[2];
};

struct DevMaterial {            // Material.hpp:6-16
    float albedo[3];
    int32_t texture_width;
    int32_t texture_height;
    uint32_t texture_pitch;
    const uint8_t* texture;
    float roughness, metallic;  // read only by the extension kernel (dead in the reference)
};

constexpr int kMaxViewInstances = 8;    // scenes of more instances render without view records (RenderParams::view_inst_off)
// Ray header of one (frame, instance) of a launch that renders through view records: what a wave of render_kernel<.., VIEW> needs
// of the instance before its loop and what does not depend on the lane, in one 64-byte block that the wave fetches through the
// scalar cache.  Written by view_records_kernel in front of the frame's view records (block i of the frame's view = instance i).
struct RayHeader {
    float ro[3];                // the frame's origin in the instance's mesh space: to_mesh_space(..).ro, the bits the view records hold
    uint32_t flags;             // kRay* below
    Q4 q_rot;                   // DevInstance::q_rot, inv_scale: the direction's transform stays per lane
    float inv_scale[3];
    int32_t root_ref;
    float inv_pose_xyz[3];
    uint32_t vdelta;            // view_base + frame * view_frame_stride + view_inst_off[i]
};
static_assert(sizeof(RayHeader) == 64, "one scalar fetch of sixteen words");
constexpr uint32_t kRayOriginFinite = 1, kRayBoxUnordered = 2, kRayExactUv = 4, kRayUnitInv = 8;

constexpr int kMaxBatch = 32;   // frames per launch (rt_render_batch); 32 x 96 B of per-frame parameters keep the kernel
                                // arguments under the 4 KB limit

struct FrameParams {            // what differs between the frames of one batched launch
    float kinv[9];
    float D[4];
    float origin[3];
    Q4 q_cam;                   // euler2quat(inv_camera_pose ypr), raycast.cu:185
    uint8_t* img;
    // stripes: whose stripes this frame's launch renders and how many rows they have.  Both are the launch's own (RenderParams::rank,
    // local_rows) unless the stripe owner ROTATES with the frame index (rt_render_stripes_batch_rotating): a rank then renders every
    // stripe class in turn, so the ranks' shares of a group of frames are equal whatever the frame shows
    int32_t rank, local_rows;
};

struct RenderParams {
    int32_t width, height;
    int32_t num_frames;         // grid.z of un-ordered primary launches; a factor of the ordered ones' grid.x
    FrameParams frames[kMaxBatch];
    const float4* records;      // interior-node and triangle records (64 B each), one index space
    const float* tri_uv;        // [slot][3][2]
    const int32_t* tri_id;      // [slot] -> caller's triangle index within its mesh
    const int32_t* leaf_count;  // [slot] count of the leaf that starts at slot (only read for count > 30)
    const int32_t* mesh_flags;  // [mesh] bit 0: some interior record of the mesh holds a box with min > max or a NaN (kBoxUnordered)
    const DevInstance* instances;
    const DevMaterial* materials;
    int32_t num_instances;
    int32_t stack_depth;        // LDS stack entries per lane
    uint64_t pitch;
    // stripes: local row ly is frame row ((ly / stripe_rows) * num_ranks + rank) * stripe_rows + ly % stripe_rows
    int32_t local_rows, stripe_rows, rank, num_ranks;   // (local_rows = the most rows any frame of the launch has: the grid's height)
    int32_t tiles_x, tiles_y;   // 16x16-pixel workgroup tiles over width x local_rows
    unsigned long long* trace;  // diagnostics: per-wave {start, end, hw id, tile} stamps, or null
    // single-frame launches (render_kernel<.., ORDERED>): heavy-tiles-first dispatch from the previous frame's costs
    const int32_t* tile_order;  // workgroup b renders tile tile_order[b] (null = b)
    int32_t* tile_cost;         // [tile] loop iterations of the tile's longest lane (null = not recorded)
    // extension kernel (rt_render_ex): samples per pixel, specular bounces, sun + shadow pass, optional pops plane
    int32_t spp, bounces, lighting;
    int32_t sample_base;        // this launch renders sample indices sample_base + blockIdx.y
    float4* ex_samples;         // [chunk][local_rows * width] radiance xyz + node pops (int bits) of one sample
    float4* ex_acc;             // [local_rows * width] running sums between chunks
    int32_t* total_pops;
    // render_ex_kernel<.., PX>: the samples of a pixel share a wave (64 lanes = px_pw x px_ph pixels x px_n sample slots)
    int32_t px_n, px_count;     // sample slots per pixel in a wave (4..64, a power of two), samples of this launch (<= px_n)
    int32_t px_pw, px_ph;       // pixels of a wave; a workgroup is 2 x 2 waves
    int32_t px_first, px_last;  // first / last chunk of the frame's samples (running sums wait in ex_acc in between)
    // render_kernel<.., VIEW>: the view record of interior record `e` of instance i in frame f is at byte offset
    // view_base + f * view_frame_stride + view_inst_off[i] + e * 64 from `records` (32-bit arithmetic; RtScene::ViewPool); the ray
    // header of instance i in frame f is at view_base + f * view_frame_stride + i * 64
    uint32_t view_base, view_frame_stride;
    int32_t view_inst_off[kMaxViewInstances];
    unsigned long long* loop_stats;     // render_kernel<.., STATS> (rt_scene_loop_stats): RT_LOOP_WORDS counters, null in every other launch
    // parity planes (tight [height][width], frame coordinates), any may be null
    int32_t *hit_instance, *hit_triangle, *node_pops, *aabb_tests, *tri_tests, *inside_hits;
    // render_kernel<.., VIEW, ., TABLE>: the launch's camera-space ray directions (camera_space_direction of every pixel, the same in
    // every frame because the frames share K_inv and D bit for bit), written by the view pre-pass into the view slot's own buffer.
    // Tile-major: component c of lane l of 8x8 tile (tx, ty) is float ((ty * tiles_x + tx) * 3 + c) * 64 + l.  Null in every other launch.
    // (The last field: no other field's offset in the kernel arguments moved when it was added.)
    const float* dir_table;
};

static_assert(sizeof(RenderParams) <= 4096, "kernel arguments must fit in 4 KB");

}  // namespace rt
