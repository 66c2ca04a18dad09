/*
 * rt_hip.h -- C-ABI of librt_hip.so: the MI355X (gfx950) raycast hot path.
 *
 * This is the drop-in boundary for the reference's per-pixel raycast.  The reference has no
 * FFI layer; its boundary is the host C++ that uploads the scene and launches the one
 * kernel.  Each entry point below names the reference interface it replaces (paths relative
 * to AFIDclan/cuda-raytracing CudaRaytracer/).  Plain pointers and sizes only; no C++ or
 * torch types; every function returns 0 on success, a positive hipError_t, or a negative
 * RT_E_* code, and never throws.  The caller owns image buffers; the library owns scene
 * buffers.  All `stream` arguments are a hipStream_t passed as void* (NULL = default stream).
 *
 * Environment (diagnostics and tests only): RT_TRACE_FILE=<path> makes every render launch synchronise and write
 * per-wave start / end stamps there (tools/trace_one.py), with RT_TRACE_PROF=1 through a stamped copy of the kernel;
 * RT_EX_SCRATCH_BYTES=<n> overrides the scratch budget of rt_render_ex (forces the chunked path);
 * RT_TILE_ORDER=0 turns the heavy-first dispatch order of single-frame launches off; RT_BVH_LIBRARY_SCAN=1 makes
 * rt_bvh_build use the partition path of meshes above 1 M triangles; RT_BVH_DEBUG=1 prints its phase timings;
 * RT_BVH_SMALL=k (0..64) lowers the size of the subtrees one wave finishes on its own (0: level loop only; tests);
 * RT_RCCL_LIBRARY=<path> makes rt_comm_* load that library instead of librccl.so.1 (tests: an in-process mock); if it cannot
 * be loaded or lacks an entry point, rt_comm_* fail with RT_E_COMM (rt_comm_last_error() has the loader's message);
 * RT_RENDER_OVERLAP=0 makes rt_render_overlapped a plain default-stream launch; RT_TILE_SORT_INTERVAL=<n> sorts a new heavy-first
 * order every n-th single-frame launch (default 4: the events that order a sort behind the launches it must wait for are recorded only then); while RT_TEST_FAIL_UPLOAD=1 is set every rt_scene_upload fails with
 * RT_E_NOMEM before it touches anything (tests of the callers' error paths).
 * Round 6: RT_OVERLAP_PRIORITY=0 gives rt_render_overlapped two streams of equal priority (see there); RT_TILE_ORDER_STRIPES=0 keeps a
 * rank's thin striped batches in natural tile order; RT_VIEW_MAX_BYTES=<n> bounds a scene's view pool (default 1 GiB, see
 * rt_scene_reserve_views).
 */
#ifndef RT_HIP_H
#define RT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 2

enum {
    RT_OK = 0,
    RT_E_INVALID = -1,      /* bad argument (null pointer, size, index out of range) */
    RT_E_NOMEM = -2,
    RT_E_DEPTH = -3,        /* BVH deeper than 64 levels (the reference's traversal stack holds 32 entries, raycast.cu:54) */
    RT_E_NODEVICE = -4,
    RT_E_COMM = -5          /* RCCL could not be loaded or returned an error: see rt_comm_last_error() */
};

/* One mesh as the reference uploads it: MeshPrimitive::to_device (MeshPrimitive.cpp:17-36) sends
 * the TrianglePrimitive array (TrianglePrimitive.hpp:8-11) and BVHTree::compile_tree
 * (BVHTree.hpp:364-383) the d_BVHTree array (BVHTree.hpp:18-26) plus one index list per leaf
 * (BVHTree.hpp:97-111).  Here the same data arrives flattened; the library re-lays it out for
 * the GPU (see DESIGN.md "Data layout in HBM").  All pointers are HOST pointers.
 *
 * The tree may be the caller's own.  What rt_scene_upload asks of it: node 0 is the root, the two children of an interior node are
 * different nodes with higher indices than their parent, every node has one parent, leaf ranges lie inside leaf_indices and
 * hold triangle indices of this mesh (anything else: RT_E_INVALID), and the tree has at most 64 levels, the root being level 1
 * (deeper: RT_E_DEPTH).  Every box must contain the vertices of the triangles below its node; it may be looser than exact.
 * Nodes may be numbered in any order that keeps children behind parents, children may stand in either slot, a leaf may hold any
 * number of triangles (the root may be a leaf, a leaf may be empty), and an empty leaf may carry an inverted box (min > max):
 * such a mesh is traversed without pruning (rt_scene_mesh_flags bit 0).  Query answers do not depend on the tree
 * (tests/test_gpu_caller_trees.py) -- with the one condition the reference's cast brings along for rt_trace_rays, rt_occluded and
 * the renders: it prunes a box by comparing the box's ray PARAMETER with the world DISTANCE of the closest hit so far, which is
 * conservative for directions of length >= 1 only, and of equal distances the first visited wins; a ray with a shorter direction,
 * or with two equal smallest distances, may find another triangle under another tree, as it may in the reference.
 * Leaf ranges may overlap, and leaf_indices may name a triangle more than once.  A triangle is then reported once per leaf
 * that references it: it counts that often in rt_count_in_boxes, rt_count_sections, rt_count_in_regions, rt_count_intersecting
 * and rt_count_crossings (and its winding), and stands that often in their lists, in rt_list_nearby and in the cells of
 * rt_occupancy_grid.  The minimum-type answers (rt_trace_rays, rt_occluded, rt_closest_points, rt_closest_to_segments,
 * rt_closest_to_triangles: distance, instance, triangle, location) are those of the mesh without the repeats.  A refit moves
 * every reference; rt_scene_rebuild_mesh_device replaces the tree by the library's own, which has none. */
typedef struct RtMeshDesc {
    int32_t num_triangles;
    const float *vertices;          /* [num_triangles][3][3]  TrianglePrimitive::vertices      */
    const float *normals;           /* [num_triangles][3]     TrianglePrimitive::normal        */
    const float *uvs;               /* [num_triangles][3][2]  TrianglePrimitive::uv_coords     */
    int32_t num_nodes;              /* node 0 is the root (MeshPrimitive.cpp:51).  0 = no tree given (the node and leaf
                                     * arrays are ignored): rt_scene_upload builds the reference's tree on the device,
                                     * in place -- the shortest way from triangles to a renderable scene            */
    const float *node_bounds;       /* [num_nodes][6]  min.xyz, max.xyz (d_BVHTree::min/max)   */
    const int32_t *node_children;   /* [num_nodes][2]  child_index_a/b; -1,-1 for a leaf       */
    const int32_t *node_leaf_first; /* [num_nodes]     offset of the leaf's list in leaf_indices */
    const int32_t *node_leaf_count; /* [num_nodes]     d_BVHTree::count_triangles (0 if interior) */
    int32_t num_leaf_indices;
    const int32_t *leaf_indices;    /* concatenated d_BVHTree::triangle_indices lists          */
} RtMeshDesc;

/* Material (Material.hpp:6-16).  texture = host BGR bytes (as cv::imread gives them,
 * Material.hpp:32) or NULL; texture_width == 0 selects the albedo path (raycast.cu:224). */
typedef struct RtMaterialDesc {
    float roughness;
    float albedo[3];
    float metallic;
    float illumination;
    const uint8_t *texture;
    int32_t texture_width, texture_height;
    size_t texture_pitch;
} RtMaterialDesc;

/* MeshInstance (MeshInstance.hpp:6-18), same field order and meaning; the inverse fields are
 * what MeshInstance::build_inv (MeshInstance.hpp:39-46) produces. */
typedef struct RtInstanceDesc {
    int32_t mesh_index;
    int32_t material_index;
    float pose[6];           /* lre: x y z yaw pitch roll (transforms.hpp:10-14) */
    float inv_pose[6];
    float rotation[3];
    float inv_rotation[3];
    float scale[3];
    float inv_scale[3];
} RtInstanceDesc;

typedef struct RtSceneDesc {
    int32_t num_meshes;     const RtMeshDesc *meshes;
    int32_t num_materials;  const RtMaterialDesc *materials;
    int32_t num_instances;  const RtInstanceDesc *instances;
} RtSceneDesc;

/* The by-value arguments of render<<<>>> (raycast.h:13, Camera.cu:23-36). */
typedef struct RtCameraParams {
    int32_t width, height;
    float K_inv[9];          /* row-major float3x3, invert_intrinsic(K) (utils.hpp:142) */
    float D[4];
    float camera_pose[6];    /* lre */
    float inv_camera_pose[6];/* invert_lre(camera_pose), Camera.cu:21 */
} RtCameraParams;

/* Optional per-pixel parity planes, tight [height][width] int32 DEVICE buffers, any may be NULL.
 * hit_* are -1 on a miss; counts follow raycast.cu:61 (pops), :69-70 (aabb tests), :86
 * (triangle tests), :96 (inside hits). */
typedef struct RtDebugPlanes {
    int32_t *hit_instance, *hit_triangle, *node_pops, *aabb_tests, *tri_tests, *inside_hits;
} RtDebugPlanes;

typedef struct RtScene RtScene;

/* ---- device / memory plumbing (replaces the cudaMallocPitch / cudaMemcpy / cudaFree /
 *      cudaDeviceSynchronize calls of kernel.cu:247-253,279,299) ------------------------------ */
int rt_abi_version(void);
/* "RT_CODE_HASH=<16 hex digits>": the hash of the kernel sources and compiler flags this library was built from, as
 * cuda-raytracing_amd/_build.py kernel_code_hash() computes it ("built-without-it" for a build that did not pass
 * -DRT_CODE_HASH).  A profile or a roofline fraction describes one build of the kernels: bench.py prices its line with the hash
 * of the library that RAN, and the Python loader refuses a library that was not built from the sources next to it. */
const char *rt_build_info(void);
int rt_device_count(int *count);
int rt_set_device(int device);
int rt_malloc(void **dptr, size_t bytes);
int rt_malloc_pitch(void **dptr, size_t *pitch, size_t width_bytes, size_t height);
int rt_free(void *dptr);
int rt_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int rt_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int rt_memcpy2d_d2h(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, void *stream);
int rt_stream_synchronize(void *stream);
int rt_device_synchronize(void);
const char *rt_error_string(int code);

/* ---- scene (replaces Scene::upload_to_device, Scene.cpp:25-65, and everything it calls) ---- */
int rt_scene_upload(const RtSceneDesc *desc, RtScene **out);
/* Scene::update_mesh_instance (Scene.cpp:67-74): re-upload one instance */
int rt_scene_update_instance(RtScene *scene, int32_t index, const RtInstanceDesc *instance);
/* the same update ordered on `stream` instead of synchronising with the device: renders issued on that stream before the
 * call see the old instance, renders issued after it the new one -- an animated instance (the teapot of kernel.cu:272-273)
 * then costs no host wait per frame.  Renders in flight on OTHER streams are not ordered against it. */
int rt_scene_update_instance_async(RtScene *scene, int32_t index, const RtInstanceDesc *instance, void *stream);
/* Refit of a deforming mesh: the same triangles (same count, same order as at upload) at new positions.  vertices
 * [n][3][3] and normals [n][3] are HOST arrays in the RtMeshDesc layout; uvs and the tree's topology stay.  Every node
 * gets the exact bounds of its triangles (what BVHTree::fill's bounds pass, BVHTree.hpp:206-209, would compute for that
 * node), triangle records are recomputed as at upload.  Ordered on `stream`: renders issued on it before the call see the
 * old mesh, renders after it the new one; the host arrays must stay valid until the stream has passed the call
 * (rt_stream_synchronize, or any later synchronising call).  Host-array refits of one scene on different streams (of different
 * meshes) are ordered against each other by the library; renders on other streams are still not ordered against a refit.
 * No counterpart in the reference. */
int rt_scene_refit_mesh(RtScene *scene, int32_t mesh_index, const float *vertices, const float *normals,
                        int32_t num_triangles, void *stream);
/* the same with DEVICE arrays (a deformation computed on the GPU: skinning, simulation): no copy, the arrays are read by
 * kernels ordered on `stream` and must stay untouched until the stream has passed them */
int rt_scene_refit_mesh_device(RtScene *scene, int32_t mesh_index, const float *d_vertices, const float *d_normals,
                               int32_t num_triangles, void *stream);
int rt_scene_destroy(RtScene *scene);
/* bytes of device memory the scene holds, and the traversal-stack depth it needs */
int rt_scene_info(const RtScene *scene, size_t *device_bytes, int32_t *max_stack);
/* per-mesh state bits kept on the device (a small synchronous copy).  Bit 0 (1): some interior record of the mesh holds a child box
 * with min > max or a NaN (an empty leaf of a degenerate split, non-finite vertices): the mesh is traversed with the generic slab
 * test instead of the octant-specialised loops (4-7 % slower on c2, same results).  Decided at upload and by every rebuild and
 * refit of the mesh. */
int rt_scene_mesh_flags(RtScene *scene, int32_t mesh_index, int32_t *flags);
/* the largest triangle count rt_scene_rebuild_mesh_device accepts for this mesh (= the count it was uploaded with: its part of
 * the record arrays has room for any tree over that many triangles) */
int rt_scene_mesh_capacity(const RtScene *scene, int32_t mesh_index, int32_t *max_triangles);

/* Device-resident rebuild of one mesh of an uploaded scene: a NEW tree (the reference's, node for node, as rt_bvh_build gives
 * it) over the n triangles in DEVICE arrays d_vertices [n][3][3], d_normals [n][3] and d_uvs [n][3][2] (NULL = all zero), n at
 * most the triangle count the mesh was uploaded with.  The build kernels and an emit pass write straight into the scene's
 * record arrays -- what rt_bvh_build + Scene::upload_to_device + rt_scene_upload produce for the same triangles, bit for bit,
 * without a host copy of vertices, tree or records: for a mesh whose motion has outgrown refitting, or whose triangles change.
 * Ordered on `stream` like rt_scene_refit_mesh_device; the call returns when the new tree is in place (it reads a few words
 * of build state back while it runs).  Replaces MeshPrimitive::build_bvh + Scene::upload_to_device (MeshPrimitive.cpp:38-56,
 * Scene.cpp:25-65) for that mesh.
 * Errors: RT_E_INVALID for a bad index or more triangles than rt_scene_mesh_capacity() -- nothing has been touched then.  A
 * HIP error after the rebuild has started (the mesh's records are cleared first) returns once `stream` has drained, and
 * leaves the mesh WITHOUT a valid tree: do not render it until a later rebuild (or a fresh rt_scene_upload) has succeeded. */
int rt_scene_rebuild_mesh_device(RtScene *scene, int32_t mesh_index, const float *d_vertices, const float *d_normals,
                                 const float *d_uvs, int32_t num_triangles, void *stream);
/* tests: copies one of the scene's device arrays to the host (which: 0 records [float4], 1 tri_uv, 2 tri_id, 3 leaf_count,
 * 4 instances); *bytes receives its size, nothing is copied when capacity is smaller */
int rt_scene_debug_read(RtScene *scene, int32_t which, void *host_dst, size_t capacity, size_t *bytes);

/* ---- GPU build of the reference's BVH (replaces MeshPrimitive::build_bvh -> BVHTree::fill(1, 32), MeshPrimitive.cpp:38-56,
 *      BVHTree.hpp:203-292): identical topology, bounds and pre-order node numbering, built level by level on the device.
 *      vertices: HOST [n][3][3].  Outputs are HOST arrays sized for 2n nodes (n leaf indices) in the RtMeshDesc layout;
 *      *num_nodes receives the node count, *num_levels (optional) the tree depth in levels. ------------------------------ */
int rt_bvh_build(const float *vertices, int32_t n, int32_t max_depth, float *node_bounds, int32_t *node_children,
                 int32_t *node_leaf_first, int32_t *node_leaf_count, int32_t *leaf_indices, int32_t *num_nodes,
                 int32_t *num_levels);

/* ---- render (replaces Camera::render_scene -> render<<<grid, block>>>, Camera.cu:18-41,
 *      raycast.cu:146-297).  d_img is a caller-owned DEVICE buffer of `height` rows of `pitch`
 *      bytes, 3 bytes per pixel in uchar3 .x .y .z order (raycast.cu:292-294).  Asynchronous on
 *      `stream` unless synchronize != 0 (Camera.cu:38-39). ------------------------------------- */
int rt_render(RtScene *scene, const RtCameraParams *cam, uint8_t *d_img, size_t pitch, void *stream, int synchronize);
/* Camera::render_scene(scene, img, pitch) with synchronize = false, as the reference's frame loop calls it: twice, into two
 * images, before one cudaDeviceSynchronize (kernel.cu:277-279).  Ordered like a launch on the DEFAULT stream against
 * everything the caller does on the default stream or device-wide -- copies and memsets of the image, rt_memcpy_*,
 * rt_scene_update_instance[_async] / refit / rebuild with a NULL stream, rt_render* with a NULL stream, rt_device_synchronize:
 * what was issued before is seen by the frame, what is issued after sees the frame -- but two consecutive calls that write
 * DIFFERENT images may overlap: they alternate between two blocking streams the scene owns, so that one frame's costly tiles
 * fill the chip while the previous frame's last workgroups drain (c2: 0.146 -> 0.13 ms per frame in the reference's loop).
 * Calls whose images share memory run in call order (the later frame wins).  Not implied, unlike a real default-stream launch:
 * ordering against work on OTHER blocking streams of the application; a caller with such streams passes its stream to
 * rt_render instead.  RT_RENDER_OVERLAP=0 makes this call rt_render(.., NULL, 0).
 * Round 6: the first of the two streams has the HIGHER stream priority, and the frame issued when it is idle -- the first frame after
 * a synchronise -- goes there: two equal streams share the chip, both frames of a pair run at half speed and end TOGETHER, so neither
 * tail is hidden (245 us for the pair, 125 us for a frame alone); with priorities the first frame takes the chip and the second fills
 * the slots its tail leaves free (the reference's loop on c2: 0.136 -> 0.131 ms per frame).  Side effect, measured on this runtime:
 * once a high-priority stream exists in the process, two NORMAL streams that alternate single frames run 11 % slower (0.112 -> 0.125 ms
 * per frame) -- an application that does both uses RT_OVERLAP_PRIORITY=0 (two equal streams, round 5's behaviour). */
int rt_render_overlapped(RtScene *scene, const RtCameraParams *cam, uint8_t *d_img, size_t pitch);
/* how many frames went through rt_render_overlapped on this scene and how many of them had to wait for the other stream
 * (an image overlapping one written there and one written here); either pointer may be NULL */
int rt_render_overlapped_stats(const RtScene *scene, uint64_t *launches, uint64_t *cross_stream_waits);
/* View records (round 5; no counterpart in the reference, whose kernel subtracts the ray origin from every box at every visit,
 * BVHTree.hpp:40-54 through raycast.cu:69-70): launches of at least four frames whose frames bring enough rays first write, per
 * frame and instance, the interior records with `box - origin` in place of the boxes (the same fp32 subtraction, done once), and
 * the traversal reads those.  Nothing in a frame depends on it; RT_VIEW_RECORDS=0 turns it off.
 * MEMORY AND BLOCKING (round 6).  The views live behind the scene's records in ONE allocation (a lane's fetch stays one 32-bit offset
 * from one base): a pool of one to three slots (launches in flight on different streams), each of `frames` views of
 * 64 B x (interior-record capacity of the largest mesh) x instances -- for the 70k-triangle c2 scene 4.2 MB per frame, 403 MB for three
 * slots of 32 frames beside 8.7 MB of records; for a 260k-triangle mesh 16.7 MB per frame.  The pool never exceeds RT_VIEW_MAX_BYTES
 * (default 1 GiB; slots are dropped, three -> two -> one, before frames are); a launch that finds no room or no free slot renders
 * without views -- same pixels (`fallbacks` below).
 *   - An application that batches says so once: rt_scene_reserve_views(scene, frames_per_launch) right after rt_scene_upload sizes
 *     the pool for launches of up to that many frames (it re-allocates the record array: call it while nothing renders the scene).
 *     Launches never grow a reserved pool: no render call blocks.  frames_per_launch = 0 hands sizing back to the launches.
 *     RT_E_NOMEM: not within the budget; RT_E_INVALID: the scene cannot use views (more than eight instances, RT_VIEW_RECORDS=0).
 *   - Without a reservation the pool grows inside the first qualifying launch that brings more frames than a slot holds, to the
 *     next of 4 / 8 / 16 / 32 frames: THAT CALL BLOCKS until the device is idle (hipDeviceSynchronize: every stream of the process),
 *     allocates, copies the records and frees the block they were in -- at most four times in a scene's life.  Render calls are
 *     otherwise asynchronous.
 * rt_scene_view_stats reports how many launches qualified, how many of those rendered without views after all, how often the pool
 * was (re)sized, and the frames a slot holds now; rt_scene_memory the bytes: the record array proper, the pool behind it, everything
 * the scene holds on the device, and the pool's shape.  Any pointer may be NULL. */
int rt_scene_reserve_views(RtScene *scene, int32_t frames_per_launch);
int rt_scene_memory(RtScene *scene, size_t *records_bytes, size_t *view_pool_bytes, size_t *device_bytes, int32_t *view_slots,
                    int32_t *view_slot_frames);
int rt_scene_view_stats(RtScene *scene, uint64_t *launches, uint64_t *fallbacks, uint64_t *grows, int32_t *slot_frames);
/* Back-facing leaves (no counterpart in the reference, which visits them).  In the views of primary and G-buffer launches -- the
 * kernels that report no visit counts -- a leaf child of one to four triangles gets a box no ray passes (NaN words) when none of its triangles
 * can be accepted from the frame's origin: (v0 - origin) . n >= 2^-20 for each of them, evaluated with the traversal's own fp32
 * operations.  Frames and hit ids are bit for bit what they were; the kernels visit fewer nodes than the
 * reference.  RT_VIEW_CULL=0 (read once per process) writes every view with the boxes as they are.
 * rt_scene_view_cull_stats (diagnostics; it waits for the device) counts, in the views that the scene's last pre-pass wrote,
 * the culled leaf children of each frame: *frames = the frames of that launch, or 0 when it wrote no culled views (none yet, the
 * switch, a launch of the samples-only extension kernel); culled_leaves[k] for k < *frames, room for 32 entries. */
int rt_scene_view_cull_stats(RtScene *scene, int32_t *frames, uint64_t *culled_leaves);
/* Direction tables (no counterpart in the reference, whose kernel derives every pixel's ray from K_inv and D in every frame,
 * raycast.cu:159-182).  A primary launch that renders through view records, for one rank, of at least two frames whose K_inv and D
 * are equal BIT FOR BIT in every frame (memcmp, so a NaN equals itself and -0 differs from 0), reads each pixel's camera-space
 * direction -- the ray up to the camera's rotation -- from a table that the view pre-pass of that same launch wrote with the kernel's
 * own function: the bits a lane would have computed, once per launch instead of once per frame.  Nothing is kept from one launch to
 * the next.  Any other launch renders as before, same pixels; RT_DIR_TABLE=0 (read once per process) turns tables off.
 * MEMORY AND BLOCKING.  Each of the pool's one to three slots owns one buffer outside the record allocation: 12 bytes per pixel of
 * whole 8x8 tiles (24.9 MB at 1920x1080), freed with the scene.  They are reported HERE (out[3]) and not in rt_scene_memory's
 * device_bytes, which stays the scene's arrays + records + view pool.  A slot's buffer grows
 * inside the first launch that brings a larger image: that call waits on the host until the slot's previous launch has finished,
 * allocates and frees -- once per slot and image size that exceeds every earlier one.  A launch that cannot allocate renders without.
 * out[0] launches that read a table, out[1] launches that rendered through view records without one, out[2] how often a slot's
 * buffer was replaced by a larger one, out[3] bytes the buffers hold now. */
int rt_scene_dir_table_stats(RtScene *scene, uint64_t out[4]);
/* Which traversal loop ran (round 6; diagnostics, no counterpart in the reference).  The primary kernel picks, per wave and
 * instance, the hand-written gfx950 loop (any instance without the exact-uv mode, when the wave's rays share a sign octant and
 * the mesh's boxes are ordered), the compiler's octant-specialised loop, or the compiler's generic loop; a tree deeper than the LDS
 * part of the stack is traversed optimistically and the lanes that outgrow it are traced again on the general stack.  Parity tests
 * pass on any of them, so a change that pushes a scene off the fast loop would only show as a slower frame: this call renders the
 * batch exactly as rt_render_batch would (same launch decisions: stack form, view records) through an INSTRUMENTED copy of the
 * kernel -- never the timed one -- waits for it, and fills stats[RT_LOOP_WORDS] (host): counts of waves x instances per loop.
 * The frames are written as by rt_render_batch. */
enum {
    RT_LOOP_WAVES = 0,          /* waves that rendered at least one pixel */
    RT_LOOP_ASM = 1,            /* wave x instance casts on the hand-written loop ... */
    RT_LOOP_ASM_POSED = 2,      /* ... of which: instances that scale or rotate (the candidate block's out-of-line transform) */
    RT_LOOP_CPP_OCTANT = 3,     /* casts on the compiler's octant-specialised loop (exact-uv meshes) */
    RT_LOOP_CPP_GENERIC = 4,    /* casts on the compiler's generic loop (mixed octants in the wave, zero / non-finite direction inverses, unordered boxes) */
    RT_LOOP_DEEP = 5,           /* casts traced again on the general stack (some lane outgrew the LDS part) */
    RT_LOOP_RETRACED_LANES = 6, /* rays (lanes) traced again */
    RT_LOOP_CPP_ITERS = 7,      /* loop iterations of all lanes on the compiler's loops (octant, generic, deep): nodes and triangles visited there */
    RT_LOOP_WORDS = 8
};
int rt_scene_loop_stats(RtScene *scene, const RtCameraParams *cams, uint8_t *const *d_imgs, size_t pitch, int32_t count,
                        void *stream, uint64_t *stats);
/* `count` (1..RT_MAX_BATCH) frames of the same size in ONE launch: cams[i] is rendered into d_imgs[i].  A frame
 * stream rendered this way keeps the GPU full while the last long rays of one frame finish (the reference's own
 * loop issues two renders before it synchronises, kernel.cu:277-279).  Asynchronous on `stream`, with one exception: a launch of four
 * or more frames that has to grow the scene's view pool blocks until the device is idle (see rt_scene_reserve_views, which avoids it).
 * MEMORY: when every frame of such a launch carries the same K_inv and D, the launch also keeps a direction table in its view slot --
 * 12 bytes per pixel of whole 8x8 tiles per slot, up to three slots (24.9 MB each at 1920x1080), outside the view pool's budget; the
 * first launch of a slot with a larger image than the slot has seen waits, on the host, for that slot's previous launch before it
 * replaces the buffer (see rt_scene_dir_table_stats; RT_DIR_TABLE=0 renders without).
 * Host threads: calls on ONE scene are serialised while they prepare and queue their launch (a few microseconds; the GPU work of
 * different streams still overlaps); different scenes do not meet. */
#define RT_MAX_BATCH 32
int rt_render_batch(RtScene *scene, const RtCameraParams *cams, uint8_t *const *d_imgs, size_t pitch, int32_t count,
                    void *stream, int synchronize);
/* the same production kernel as rt_render, additionally storing the accepted hit of every pixel (raycast.cu:107-127):
 * tight [height][width] int32 DEVICE planes, -1 on a miss, either may be NULL.  For parity tests of the kernel that is
 * actually timed (rt_render_debug runs an instrumented copy). */
int rt_render_ids(RtScene *scene, const RtCameraParams *cam, uint8_t *d_img, size_t pitch, int32_t *d_hit_instance,
                  int32_t *d_hit_triangle, void *stream, int synchronize);
/* ---- G-buffer frames: what the primary ray of every pixel of `count` (1..RT_MAX_BATCH) cameras of one size
 *      hits, as planes, in ONE launch of the primary kernel's G-buffer form -- the range, depth, position, normal, uv and ids a
 *      depth camera, a range scanner or a dataset generator wants of a calibrated camera, without the detour through
 *      rt_camera_rays + rt_trace_rays.  For pixel (x, y) of frame i:
 *      1. Every plane but `depth` holds, bit for bit, what rt_trace_rays gives for ray y * width + x of rt_camera_rays(&cams[i]):
 *         the reference's cast_ray on the reference's camera ray, quirks included (see "ray queries" below: t is a world
 *         DISTANCE, back faces are never hit, of equal distances the first visited wins).
 *      2. depth = apply_lre(camera_pose_i, location).z, one fixed fp32 sequence without contraction: with q = euler2quat(yaw,
 *         pitch, roll of camera_pose_i) (transforms.hpp:148-163, on the host) and v = location - camera position per component,
 *         apply_quat(q, v) of transforms.hpp:165-176 -- a = -v.x*q.y - v.y*q.z - v.z*q.w, b = v.x*q.x + v.y*q.w - v.z*q.z,
 *         c = v.y*q.x + v.z*q.y - v.x*q.w, d = v.z*q.x + v.x*q.z - v.y*q.y, left to right -- and
 *         depth = q.x*d - q.w*a - q.y*c + q.z*b, left to right (the quaternion is stored (w, x, y, z) in .x .y .z .w).
 *         FLT_MAX on a miss.  It is the hit's coordinate along the z axis of the frame camera_pose defines, not a distance
 *         (that is `t`) and not a coordinate along the viewing direction (raycast.cu:182 looks along that frame's +y).
 *      3. Layout: tight DEVICE planes, frame-major; the element of pixel (x, y) of frame i is (i * height + y) * width + x, times
 *         3 (location, normal) or 2 (uv) for the vector planes.  Every offset is computed in size_t.
 *      d_imgs: NULL = no colour frames (the kernel then does not shade: no texture fetch, no store); otherwise d_imgs[i] gets
 *      exactly rt_render's bytes for cams[i], rows `pitch` bytes apart.
 *      Asynchronous on `stream` unless synchronize != 0, with rt_render_batch's launch decisions (stack form; view records and
 *      the direction table for four frames or more), hence its view-pool behaviour -- a launch that has to grow the pool blocks
 *      until the device is idle, rt_scene_reserve_views avoids it -- its direction-table memory and its serialisation of host
 *      threads on one scene: see rt_render_batch above.  One rank only: no stripes; never the heavy-first tile order;
 *      RT_TRACE_FILE does not apply.  Pixels whose ray has a non-finite component (a non-finite pose) do not fault and do
 *      not change other frames; their own values are unspecified.
 *      RT_E_INVALID: NULL scene, cams or out; count outside 1..RT_MAX_BATCH; frames of different sizes (or a size < 1); no
 *      output at all (no plane and no d_imgs); a NULL entry in a non-NULL d_imgs; pitch < 3 * width with d_imgs. ------------- */
typedef struct RtGBuffer {      /* every pointer optional (NULL = not wanted); DEVICE, tight, frame-major: [count][height][width](xk) */
    float   *t;                 /* RtRayHits::t of the pixel's primary ray (HitInfo::min); FLT_MAX on a miss */
    float   *depth;             /* camera-space z of the accepted hit: apply_lre(cam.camera_pose, location).z (rule 2); FLT_MAX on a miss */
    int32_t *instance, *triangle;   /* rt_render_ids' planes; -1 on a miss */
    float   *location;          /* [..][3] RtRayHits::location; 0 on a miss */
    float   *normal;            /* [..][3] RtRayHits::normal;   0 on a miss */
    float   *uv;                /* [..][2] RtRayHits::uv;       0 on a miss */
} RtGBuffer;
int rt_render_gbuffer(RtScene *scene, const RtCameraParams *cams, int32_t count /* 1..RT_MAX_BATCH */,
                      uint8_t *const *d_imgs /* NULL = no colour frames */, size_t pitch,
                      const RtGBuffer *out, void *stream, int synchronize);
/* ---- sensor frames: the G-buffer and the colour of a sensor that is not the reference's pinhole -- a spinning
 *      lidar, an equirectangular panorama, a fisheye, a Brown-Conrady camera: any ray pattern with ONE centre of projection -- from a
 *      table of camera-space directions the caller fills.
 *      RtRayTable: a device-resident table of width x height directions in the layout the primary kernel's table form reads
 *      (tile-major, one 8x8 tile = 3 x 64 floats, x / y / z planes 64 apart; tile ty * tiles_x + tx; lane (y & 7) * 8 + (x & 7); room
 *      for whole tiles, 768 bytes each).  Immutable once created: any number of scenes, streams and host threads may use one table at
 *      once.  Its memory belongs to no scene: not in rt_scene_info / rt_scene_memory, see rt_ray_table_info.
 *      An entry c of pixel (x, y) is the vector in the camera frame after raycast.cu:182: +y the optical axis, +x image right, +z
 *      image up.  Under a pose P (camera_pose, inv_camera_pose of RtCameraParams) the pixel's ray has origin P.xyz and direction
 *      normalize3(apply_euler(inv_camera_pose.ypr, c)) -- raycast.cu:185-188, computed as the render kernels compute it, as a
 *      quaternion product with q = euler2quat(inv_camera_pose.ypr) made on the host.  Entries need not have unit length; zero
 *      components are ordinary input.  A non-finite or all-zero entry does not fault and does not change other pixels; its own values
 *      are unspecified. */
typedef struct RtRayTable RtRayTable;
/* d_dirs: DEVICE [height][width][3] floats, row-major, read on `stream` (asynchronously unless synchronize != 0: keep it alive and
 * unchanged until then).  The table holds the caller's bits unchanged; lanes beyond a ragged edge hold (0, 1, 0).
 * RT_E_INVALID: NULL d_dirs or out, a size < 1, more than 65 535 rows of tiles, more than 2^24 tiles.  RT_E_NOMEM is possible. */
int rt_ray_table_create(const float *d_dirs, int32_t width, int32_t height, void *stream, int synchronize, RtRayTable **out);
/* every out pointer optional; device_bytes = tiles_x * tiles_y * 768 */
int rt_ray_table_info(const RtRayTable *table, int32_t *width, int32_t *height, size_t *device_bytes);
/* the caller has synchronised whatever reads the table (its creation included), as with rt_free; NULL is accepted */
int rt_ray_table_destroy(RtRayTable *table);
/* The camera-space direction of every pixel of a camera (raycast.cu:159-182: K_inv, the atan distortion, the swizzle), DEVICE
 * [height * width][3], row-major: what the library's own direction tables hold.  A table created from this output makes
 * rt_ray_table_rays equal rt_camera_rays and rt_render_gbuffer_table equal rt_render_gbuffer for that camera, bit for bit. */
int rt_camera_directions(const RtCameraParams *cam, float *d_dirs, void *stream, int synchronize);
/* rt_camera_rays for a table: DEVICE origins and world directions [height * width][3], row-major.  Of `pose` only camera_pose,
 * inv_camera_pose, width and height are read (K_inv and D are ignored).  RT_E_INVALID: a NULL argument, a size that is not the table's. */
int rt_ray_table_rays(const RtRayTable *table, const RtCameraParams *pose, float *d_origins, float *d_directions, void *stream,
                      int synchronize);
/* rt_render_gbuffer with the pixel's ray taken from the table.  Rule 1 becomes: every plane but `depth` holds, bit for bit, what
 * rt_trace_rays gives for ray y * width + x of rt_ray_table_rays(table, &poses[i]); rules 2 and 3 are unchanged.  d_imgs[i] gets the
 * flat shade of that hit -- the sky colour on a miss, otherwise as rt_render -- and images alone (every plane NULL) are a valid call:
 * the colour render of a sensor.  With four frames or more (and whatever else rt_render_batch asks of a view launch) the launch
 * takes view records, otherwise plain records; both read the caller's table, the library writes none, and
 * rt_scene_dir_table_stats does not count the launch.
 * RT_E_INVALID: the cases of rt_render_gbuffer, a NULL table, a pose whose width or height is not the table's. */
int rt_render_gbuffer_table(RtScene *scene, const RtRayTable *table, const RtCameraParams *poses, int32_t count /* 1..RT_MAX_BATCH */,
                            uint8_t *const *d_imgs /* NULL = no colour frames */, size_t pitch, const RtGBuffer *out, void *stream,
                            int synchronize);
/* ---- point clouds: the compacted returns of `count` (1..RT_MAX_BATCH) camera or sensor frames of one size --
 *      only the pixels that hit something inside the range gate and the valid area, packed, with the sensor-frame coordinates and
 *      the ring / column index of each point.  The accepted hit of pixel (x, y) of frame i is exactly what rt_render_gbuffer (cameras)
 *      or rt_render_gbuffer_table (a ray table) puts in its planes for that pixel.
 *      1. Keep rule.  A pixel is kept iff instance >= 0, and t >= min_range and t <= max_range as fp32 comparisons (a NaN t is
 *         not kept; min_range = 0, max_range = +inf keeps every hit), and d_mask == NULL || d_mask[y * width + x] != 0 (d_mask:
 *         DEVICE uint8 [height][width], shared by all frames).
 *      2. Order.  Kept pixels are ordered by (i, y, x): deterministic, independent of launch form, stream or run.
 *      3. Offsets.  d_offsets: DEVICE int64 [count + 1]; d_offsets[i] = the number of kept pixels in frames < i, d_offsets[count]
 *         the total.
 *      4. Fields of point j (RtPointCloud): each optional, tight, indexed in size_t.  range = t; pixel = y * width + x (ring y,
 *         column x of a spinning lidar); frame = i; instance, triangle, position (= the location plane), normal, uv = the G-buffer
 *         planes' bits of that pixel: the numpy compaction of the plane.
 *      5. local = apply_lre(camera_pose_i, location), all three components, by rule 2 of the G-buffer frames: q = euler2quat(yaw,
 *         pitch, roll of camera_pose_i) on the host, v = location - camera position per component, a, b, c, d as there, and, each
 *         left to right in fp32 without contraction,
 *           local.x = q.x*b - q.y*a - q.z*d + q.w*c
 *           local.y = q.x*c - q.z*a - q.w*b + q.y*d
 *           local.z = q.x*d - q.w*a - q.y*c + q.z*b        (= the depth plane, bit for bit)
 *         (the quaternion is stored (w, x, y, z) in .x .y .z .w).
 *      Two steps, so that one traversal serves an exact allocation and a fully asynchronous use alike:
 *      rt_point_cloud_offsets(_table) renders the staging planes `fields` need into the caller's workspace with rt_render_gbuffer's
 *      launch (its decisions, its view-pool behaviour, its serialisation of host threads on one scene; t and instance always,
 *      triangle, normal, uv when asked, location for position or local; no images, no depth plane), counts the kept pixels per chunk
 *      of 64 consecutive pixels of a frame, scans the counts (the per-chunk offsets stay in the workspace) and writes d_offsets.
 *      Nothing of the scene is held after the launch: calls on one scene with different workspaces overlap as G-buffer calls do.
 *      rt_point_cloud_fill needs no scene: it reads the workspace -- unchanged since *_offsets, later in the same stream order, with
 *      the same cams, count and fields -- and writes point j only when j < capacity: a cloud larger than `capacity` is truncated to
 *      its first `capacity` points (d_offsets keeps the true counts), capacity = 0 writes nothing.  Of cams only width, height and
 *      camera_pose are read.  Every read is bounded by sizes derived from the arguments and every write by capacity: a stale or
 *      foreign workspace gives wrong points, never an access outside the workspace or the outputs.
 *      RT_E_INVALID, judged before any device call: the cases of rt_render_gbuffer(_table) that apply; NULL d_offsets or workspace;
 *      a workspace smaller than rt_point_cloud_workspace_bytes; fields == 0 or unknown bits; a NaN min_range or max_range, or
 *      min_range > max_range; more than 2^31 - 1 chunks; for fill also a NULL `out`, a non-NULL pointer whose bit is not in
 *      `fields` (a NULL pointer for a bit that is set is fine: not wanted), a negative capacity, no output at all. ----------- */
#define RT_CLOUD_RANGE    0x001u
#define RT_CLOUD_PIXEL    0x002u
#define RT_CLOUD_FRAME    0x004u
#define RT_CLOUD_INSTANCE 0x008u
#define RT_CLOUD_TRIANGLE 0x010u
#define RT_CLOUD_POSITION 0x020u
#define RT_CLOUD_LOCAL    0x040u
#define RT_CLOUD_NORMAL   0x080u
#define RT_CLOUD_UV       0x100u
#define RT_CLOUD_ALL      0x1ffu
typedef struct RtPointCloud {   /* every pointer optional (NULL = not wanted); DEVICE, tight, [capacity](xk); bit order of RT_CLOUD_* */
    float   *range;             /* t */
    int32_t *pixel;             /* y * width + x */
    int32_t *frame;             /* i */
    int32_t *instance, *triangle;
    float   *position;          /* [..][3] world: the location plane */
    float   *local;             /* [..][3] apply_lre(camera_pose_i, location) (rule 5) */
    float   *normal;            /* [..][3] */
    float   *uv;                /* [..][2] */
} RtPointCloud;
/* 0 for a size or count < 1, count > RT_MAX_BATCH, fields == 0 or unknown bits, or more than 2^31 - 1 chunks */
size_t rt_point_cloud_workspace_bytes(int32_t width, int32_t height, int32_t count, uint32_t fields);
int rt_point_cloud_offsets(RtScene *scene, const RtCameraParams *cams, int32_t count /* 1..RT_MAX_BATCH */, float min_range,
                           float max_range, const uint8_t *d_mask /* NULL = every pixel valid */, uint32_t fields, int64_t *d_offsets,
                           void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
int rt_point_cloud_offsets_table(RtScene *scene, const RtRayTable *table, const RtCameraParams *poses, int32_t count, float min_range,
                                 float max_range, const uint8_t *d_mask, uint32_t fields, int64_t *d_offsets, void *d_workspace,
                                 size_t workspace_bytes, void *stream, int synchronize);
int rt_point_cloud_fill(const RtCameraParams *cams, int32_t count, uint32_t fields, const void *d_workspace, size_t workspace_bytes,
                        int64_t capacity, const RtPointCloud *out, void *stream, int synchronize);
/* ---- rolling frames: sensor frames and clouds whose pixels are NOT taken from one pose -- a spinning lidar
 *      that fires its columns over a revolution while the vehicle moves, a rolling-shutter camera that exposes its rows one after
 *      another (the same call with a table made from rt_camera_directions).  A rolling frame belongs to a ray table of width x height
 *      and is defined by an axis (0: the column x selects the slice, 1: the row y does), slice_pixels, a positive multiple of 8, and
 *      slices = ceil(extent / slice_pixels) poses, extent = width for axis 0, height for axis 1.  The slice of pixel (x, y) is
 *      (axis ? y : x) / slice_pixels; the last slice may be narrower than the others.  Frame i uses poses[i * slices + s] for slice s.
 *      Slices are whole 8x8 tiles, so a wave of the primary kernel still has one origin and one rotation: slices finer than a tile
 *      (a pose per column) have no common centre per wave and stay with rt_trace_rays.
 *      1. Every plane except `depth` and `local` holds, bit for bit, what rt_trace_rays gives for the ray rt_ray_table_rays(table,
 *         pose of the pixel's slice) makes for that pixel -- the reference's quirks included, as for G-buffer and sensor frames.
 *      2. local = apply_lre(camera_pose of the pixel's slice, location): the hit in the sensor's frame at the moment the pixel was
 *         taken -- the raw, motion-distorted scan -- while `location` is the de-skewed truth in the world.  All three components by
 *         rule 5 of the point clouds (q = the host's euler2quat of that camera_pose, every sum left to right, nothing contracted);
 *         depth equals local.z bit for bit.  On a miss local is 0 and depth FLT_MAX.
 *      3. Layout, images (d_imgs, pitch) and non-finite poses as for rt_render_gbuffer_table; d_local is one more optional plane,
 *         [count][height][width][3].  A slice whose pose is non-finite may put unspecified values into its own pixels; it does not
 *         fault and does not change other slices or frames.
 *      4. A rolling launch always reads plain records: it never takes a view slot, never grows the view pool and is counted by
 *         neither rt_scene_view_stats nor rt_scene_dir_table_stats (view records are box - origin per frame and instance: a set
 *         per slice would take hundreds of times the memory).  The stack form is chosen as rt_render_gbuffer chooses it.
 *      5. RT_E_INVALID, judged before any device call: an axis that is neither 0 nor 1; slice_pixels < 8 or not a multiple of 8;
 *         NULL poses, table, workspace, scene or out; a workspace smaller than rt_rolling_workspace_bytes; count outside
 *         1..RT_MAX_BATCH; no output at all (no plane, no d_local and no d_imgs); a NULL entry in a non-NULL d_imgs; pitch <
 *         3 * width with d_imgs.
 *      poses: a HOST array [count][slices].  The call packs one 48-byte record per frame and slice -- the position, euler2quat of
 *      inv_camera_pose's and of camera_pose's angles, made on the host so that their bits are those rt_ray_table_rays uses -- and
 *      copies the records into the caller's workspace, ordered on `stream`, in front of the launch.  `poses` may be reused when the
 *      call returns.  The copy reads ordinary host memory: it may wait until the work issued EARLIER on `stream` has finished (as
 *      any copy from pageable memory), never for the render it precedes; the render itself is asynchronous unless synchronize != 0.
 *      The workspace must stay untouched until the stream has passed the render.  The scene is held for the launch only: calls on
 *      one scene with different workspaces overlap as G-buffer calls do. */
typedef struct RtRollingPose {  /* camera_pose and inv_camera_pose of RtCameraParams */
    float camera_pose[6];       /* x, y, z, yaw, pitch, roll */
    float inv_camera_pose[6];   /* invert_lre(camera_pose) */
} RtRollingPose;
/* slices = ceil((axis ? height : width) / slice_pixels).  RT_E_INVALID: a size < 1, a bad axis or slice_pixels, a NULL slices. */
int rt_rolling_slices(int32_t width, int32_t height, int32_t axis, int32_t slice_pixels, int32_t *slices);
/* count x slices records of 48 bytes, in whole 256-byte blocks; 0 for count outside 1..RT_MAX_BATCH or slices < 1 */
size_t rt_rolling_workspace_bytes(int32_t count, int32_t slices);
int rt_render_gbuffer_rolling(RtScene *scene, const RtRayTable *table, const RtRollingPose *poses /* HOST [count][slices] */,
                              int32_t count /* 1..RT_MAX_BATCH */, int32_t axis, int32_t slice_pixels,
                              uint8_t *const *d_imgs /* NULL = no colour frames */, size_t pitch, const RtGBuffer *out,
                              float *d_local /* optional [count][height][width][3] */, void *d_workspace, size_t workspace_bytes,
                              void *stream, int synchronize);
/* Rolling clouds: rt_point_cloud_offsets_table / rt_point_cloud_fill for rolling frames.  Rules 1-4 of the point clouds hold
 * unchanged; rule 5's `local` uses the camera_pose of the point's slice (= the compacted `local` plane of the rolling frame), and
 * `position` stays the world location.  The workspace is the static cloud's followed by the pose records, so the fill needs neither
 * the scene nor the poses: it is given the table's size, count, axis, slice_pixels and fields as *_offsets_rolling was.  Everything
 * read from the workspace is data: the slice index is bounded by `slices` before a record is read, the slot by `capacity` before a
 * store.  The record copy of *_offsets_rolling waits as rt_render_gbuffer_rolling's does.
 * RT_E_INVALID, judged before any device call: the cases of rt_render_gbuffer_rolling and of rt_point_cloud_offsets / _fill that
 * apply, a workspace smaller than rt_point_cloud_rolling_workspace_bytes. */
/* 0 where rt_point_cloud_workspace_bytes or rt_rolling_workspace_bytes is */
size_t rt_point_cloud_rolling_workspace_bytes(int32_t width, int32_t height, int32_t count, uint32_t fields, int32_t slices);
int rt_point_cloud_offsets_rolling(RtScene *scene, const RtRayTable *table, const RtRollingPose *poses, int32_t count, int32_t axis,
                                   int32_t slice_pixels, float min_range, float max_range, const uint8_t *d_mask, uint32_t fields,
                                   int64_t *d_offsets, void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
int rt_point_cloud_fill_rolling(int32_t width, int32_t height, int32_t count, int32_t axis, int32_t slice_pixels, uint32_t fields,
                                const void *d_workspace, size_t workspace_bytes, int64_t capacity, const RtPointCloud *out,
                                void *stream, int synchronize);
/* ---- visibility masks: is the surface a pixel sees also seen from over there?  For every pixel of staged
 *      G-buffer planes and each of 1..32 caller points per frame -- a projector, the partner camera of a stereo pair, the next pose,
 *      a point light, an antenna -- one bit: the point sees the pixel's surface hit.  The planes are tight, frame-major DEVICE planes
 *      in RtGBuffer's layout (`instance`, `location`, `normal`): the output of rt_render_gbuffer, _table or _rolling, or of
 *      rt_trace_rays reshaped.  Every offset is computed in size_t.
 *      The rule, for pixel p of frame i with instance[p] >= 0, X = location[p], L = points[i][k]; fp32, each sum left to right,
 *      nothing contracted:
 *      1. v = X - L per component.
 *      2. d = magnitude(v) of rt_math.h: sqrtf(v.x*v.x + v.y*v.y + v.z*v.z).
 *      3. s = 1.0f - bias.
 *      4. tmax = d * s.
 *      5. Bit k of visible[p] is set exactly when rt_occluded answers 0 for origin L, direction v (not normalised) and bound tmax:
 *         the library's own ray rule, quirks included -- back faces are never hit, a miss is not occluded.  The cast runs from L,
 *         not from the hit: it is the ray a camera at L casts at that surface point, and the surface's own triangle, met at
 *         about d, is excluded by the RELATIVE bias.
 *      6. w = L - X per component.
 *      7. Bit k of facing[p] is set exactly when normal.x*w.x + normal.y*w.y + normal.z*w.z > 0.  (The world is one-sided: a point
 *         behind an open sheet sees through it as a camera there would.  Callers who want "lit" take visible & facing.)
 *      8. A miss (instance < 0) gives 0 in both planes.
 *      9. Bits >= num_points are 0.
 *      A pixel whose X, or a point whose L, is non-finite, or a pair with v == 0, does not fault and does not change other pixels or
 *      bits; its own bit is unspecified.
 *      Asynchronous on `stream` unless synchronize != 0.  No scene scratch, no view records, no workspace: calls overlap each other
 *      and renders on other streams, as the ray queries do.  The library splits a call into as many launches as its grid limits need.
 *      RT_E_INVALID, judged before any device call: a NULL scene, d_instance, d_location, d_points or out; both outputs NULL; facing
 *      wanted but d_normal NULL; width, height or count < 1; width * height * count > 2^31 - 1; num_points outside 1..32; bias not
 *      finite or outside [0, 1). -------------------------------------------------------------------------------------------------- */
typedef struct RtVisibility { int32_t *visible, *facing; } RtVisibility;   /* DEVICE [count][height][width], each optional, at least one */
int rt_visibility(RtScene *scene, const int32_t *d_instance, const float *d_location, const float *d_normal /* NULL unless facing */,
                  int32_t width, int32_t height, int32_t count, const float *d_points /* DEVICE [count][num_points][3], world */,
                  int32_t num_points /* 1..32 */, float bias, const RtVisibility *out, void *stream, int synchronize);
/* same frame plus the parity planes (instrumented copy of the kernel: counts every visit) */
int rt_render_debug(RtScene *scene, const RtCameraParams *cam, uint8_t *d_img, size_t pitch,
                    const RtDebugPlanes *planes, void *stream, int synchronize);

/* ---- extension (no counterpart in the reference snapshot, whose shadow pass is commented out
 *      at raycast.cu:262-287 and which has no spp / bounce loop).  Semantics: DESIGN.md "Extension".  With
 *      spp = 1, bounces = 0, lighting = 0 the frame equals rt_render's bit for bit.  d_total_pops: optional tight
 *      [height][width] int32 device plane receiving the node pops of all rays of each pixel.  The per-sample
 *      scratch lives in the scene handle: extension renders on one scene must not overlap on different streams. -- */
typedef struct RtRenderOptions {
    int32_t spp;        /* >= 1; sample 0 is the reference's un-jittered ray, sample s > 0 is jittered from its own XORWOW
                           stream (seed = the reference's per-pixel seed + s) */
    int32_t bounces;    /* specular bounces weighted by Material::metallic, perturbed by Material::roughness */
    int32_t lighting;   /* 1 = sun + shadow ray of raycast.cu:249-287, 0 = illumination 1.0 (raycast.cu:282) */
} RtRenderOptions;
int rt_render_ex(RtScene *scene, const RtCameraParams *cam, const RtRenderOptions *opts, uint8_t *d_img, size_t pitch,
                 int32_t *d_total_pops, void *stream, int synchronize);

/* this rank's stripes of an extension frame (see rt_render_stripes below for the stripe layout) */
int rt_render_ex_stripes(RtScene *scene, const RtCameraParams *cam, const RtRenderOptions *opts, uint8_t *d_local,
                         size_t local_pitch, int32_t stripe_rows, int32_t rank, int32_t num_ranks, void *stream, int synchronize);

/* ---- frame tiling across GPUs (no counterpart in the reference: it is single-GPU).  The frame
 *      is cut into stripes of `stripe_rows` rows; stripe s belongs to rank s % num_ranks.  A rank
 *      renders its stripes into a tight local buffer (rows packed in stripe order, pitch =
 *      local_pitch); rt_stripe_rows() gives that buffer's row count for any rank. ------------- */
int rt_stripe_rows(int32_t height, int32_t stripe_rows, int32_t rank, int32_t num_ranks, int32_t *rows);
int rt_render_stripes(RtScene *scene, const RtCameraParams *cam, uint8_t *d_local, size_t local_pitch,
                      int32_t stripe_rows, int32_t rank, int32_t num_ranks, void *stream, int synchronize);
int rt_render_stripes_batch(RtScene *scene, const RtCameraParams *cams, uint8_t *const *d_locals, size_t local_pitch,
                            int32_t count, int32_t stripe_rows, int32_t rank, int32_t num_ranks, void *stream, int synchronize);
/* The same with the stripe owner ROTATING over the frames: frame i of the launch renders the stripes of owner
 * (rank + first_frame + i) % num_ranks (first_frame >= 0: the index of cams[0] within its group of frames).  The owners' shares
 * of a frame differ -- 1080 rows are 67.5 stripes of 16, so at 8 ranks three own 144 rows, four 128, and stripes near the
 * object cost more than sky -- and the slowest rank sets the pace of every exchange; with rotation every rank renders every
 * owner's share once per num_ranks frames, so the ranks' shares of a group are equal whatever the frames show (c2 at 8 ranks:
 * max / mean of the render time 1.04 -> 1.00).  Frame i's rows are packed in d_locals[i] as that owner's; the buffer must hold
 * the rows of the largest share (rt_stripe_rows of rank 0).  rt_unstripe_batch_rotating is the matching un-stripe pass. */
int rt_render_stripes_batch_rotating(RtScene *scene, const RtCameraParams *cams, uint8_t *const *d_locals, size_t local_pitch,
                                     int32_t count, int32_t stripe_rows, int32_t rank, int32_t num_ranks, int32_t first_frame,
                                     void *stream, int synchronize);
/* after a gather of every rank's local buffer (rank r's rows start at d_gathered + r * rank_stride bytes, rows
 * local_pitch bytes apart) place the rows back into frame order */
int rt_unstripe(const uint8_t *d_gathered, size_t local_pitch, size_t rank_stride,
                uint8_t *d_img, size_t pitch, int32_t width, int32_t height,
                int32_t stripe_rows, int32_t num_ranks, void *stream);

/* the same for `count` frames at once: frame f reads from d_gathered + f * src_frame_stride and writes to
 * d_imgs + f * dst_frame_stride (the layout of a gathered rt_render_stripes_batch group) */
int rt_unstripe_batch(const uint8_t *d_gathered, size_t local_pitch, size_t rank_stride, size_t src_frame_stride,
                      uint8_t *d_imgs, size_t pitch, size_t dst_frame_stride, int32_t count,
                      int32_t width, int32_t height, int32_t stripe_rows, int32_t num_ranks, void *stream);

/* rt_unstripe_batch for frames rendered by rt_render_stripes_batch_rotating: frame f of the batch has index first_frame + f in its
 * group, so the block of rank r (at d_gathered + r * rank_stride) holds the rows of owner (r + first_frame + f) % num_ranks */
int rt_unstripe_batch_rotating(const uint8_t *d_gathered, size_t local_pitch, size_t rank_stride, size_t src_frame_stride,
                               uint8_t *d_imgs, size_t pitch, size_t dst_frame_stride, int32_t count,
                               int32_t width, int32_t height, int32_t stripe_rows, int32_t num_ranks, int32_t first_frame, void *stream);

/* ---- the exchange step of frame tiling: an RCCL communicator over the GPUs of one node (no counterpart in the
 *      reference; BASELINE.json north_star: "the frame is tiled across the 8 GPUs of one node with a final RCCL gather
 *      over xGMI").  RCCL (librccl.so.1) is loaded on first use; without it these calls return RT_E_COMM.
 *      One process per GPU: rank 0 calls rt_comm_unique_id, the host application passes the 128 bytes to the other
 *      ranks by its own means (MPI, a socket, torch.distributed ...), every rank selects its device (rt_set_device)
 *      and calls rt_comm_init_rank.  One process for all GPUs: rt_comm_init_all fills comms[0..num_devices) (rank i on
 *      devices[i], or on device i when devices is NULL) and the *_all calls drive them.
 *      Collectives are asynchronous on `stream` like every other call here. ------------------------------------- */
typedef struct RtComm RtComm;
#define RT_COMM_ID_BYTES 128
int rt_comm_available(int32_t *rccl_version);            /* RT_OK when RCCL could be loaded */
const char *rt_comm_last_error(void);                    /* text of the calling thread's last RT_E_COMM */
/* text of the most recent RT_E_COMM of ANY thread of the process (for a watchdog thread that reports on a main thread stuck
 * inside a collective); the pointer is the calling thread's own copy, valid until its next call */
const char *rt_comm_last_error_any(void);
int rt_comm_unique_id(uint8_t *id /* [RT_COMM_ID_BYTES] */);
int rt_comm_init_rank(const uint8_t *id, int32_t rank, int32_t num_ranks, RtComm **out);   /* on the current device */
int rt_comm_init_all(const int32_t *devices, int32_t num_devices, RtComm **comms);
/* rank and size as the RCCL communicator itself reports them (ncclCommUserRank / ncclCommCount; the values given at creation
 * if the library lacks the two queries), and the device it lives on */
int rt_comm_info(const RtComm *comm, int32_t *rank, int32_t *num_ranks, int32_t *device);
int rt_comm_destroy(RtComm *comm);
int rt_group_start(void);                                /* ncclGroupStart / ncclGroupEnd for single-process callers */
int rt_group_end(void);
/* every rank's `bytes` bytes at d_send to rank `root`, which receives rank r's block at d_recv + r * bytes
 * (d_recv may be NULL elsewhere): the per-frame gather of SURVEY.md 8(e) */
int rt_gather(RtComm *comm, const void *d_send, size_t bytes, void *d_recv, int32_t root, void *stream);
/* rank p gets send_bytes[p] bytes from d_send + send_offsets[p]; recv_bytes[p] bytes from rank p land at
 * d_recv + recv_offsets[p] (zero-byte pairs are skipped; the counts must agree pairwise).  One fused group of
 * point-to-point transfers: the gathers of a group of frames whose root rotates over the ranks. */
int rt_all_to_all(RtComm *comm, const void *d_send, const size_t *send_bytes, const size_t *send_offsets,
                  void *d_recv, const size_t *recv_bytes, const size_t *recv_offsets, void *stream);
/* One tiled frame, the whole of SURVEY.md 8(e) in one call made by every rank: render this rank's stripes (rt_render_stripes,
 * or rt_render_ex_stripes when opts is non-NULL and not the default 1 / 0 / 0), gather them to `root`, and on the root
 * put the rows back into frame order in d_img (may be NULL on other ranks).  Scratch buffers live in the communicator:
 * consecutive calls on one RtComm may use different streams (frames alternated between two streams) -- each call waits, on its
 * stream, for the previous call's last use of the scratch (an event, no host synchronisation); calls on one RtComm from
 * several host threads at once are not supported.  With one rank this is rt_render / rt_render_ex. */
int rt_render_tiled(RtScene *scene, RtComm *comm, const RtCameraParams *cam, const RtRenderOptions *opts, uint8_t *d_img,
                    size_t pitch, int32_t stripe_rows, int32_t root, void *stream, int synchronize);
/* the same from ONE process that holds a scene replica and a communicator per device (rt_comm_init_all):
 * scenes[r] / comms[r] / streams[r] (streams may be NULL) belong to rank r; d_img is on the root's device */
int rt_render_tiled_all(RtScene *const *scenes, RtComm *const *comms, int32_t num_ranks, const RtCameraParams *cam,
                        const RtRenderOptions *opts, uint8_t *d_img, size_t pitch, int32_t stripe_rows, int32_t root,
                        void *const *streams, int synchronize);

/* ---- ray queries (replaces a call of cast_ray, raycast.cu:21-142, on rays the CALLER chooses; DESIGN.md "Ray queries").
 *      Closest hit = the reference's cast_ray(ray) bit for bit, quirks included: directions are not normalised, `t` is the
 *      Euclidean world distance from the origin to the accepted hit (HitInfo::min), not a ray parameter; back faces are never
 *      hit (same_dir < 0, :107-109); there is no t-min; a box is pruned by comparing its MESH-space distance with the world
 *      min; of equal distances the first visited wins.  Rays are DEVICE arrays [n][3] float; outputs are tight DEVICE arrays
 *      of n rows, indexed like the rays.  Rays with a non-finite component do not fault and do not change other rays'
 *      results; their own results are unspecified.  Zero direction components are ordinary input.
 *      Octant binning: with a workspace of rt_trace_workspace_bytes(n) device bytes the rays are first sorted by the sign
 *      octant of their direction (a counting sort on the device) and traced in that order -- the results are the same bit for
 *      bit, only the order of the work changes; NULL traces in input order.  A workspace serves one call at a time.
 *      Asynchronous on `stream` unless synchronize != 0; nothing is launched when n == 0.  Calls on one scene may overlap each
 *      other and renders on other streams (no scene scratch is used).  RT_E_INVALID: NULL scene, n < 0, NULL rays (or
 *      outputs) with n > 0, a non-NULL workspace smaller than rt_trace_workspace_bytes(n). ------------------------------ */
typedef struct RtRayHits {      /* every pointer optional (NULL = not wanted) */
    float   *t;                 /* HitInfo::min: world distance origin -> accepted hit; FLT_MAX on a miss               */
    int32_t *instance;          /* index into the scene's instances, -1 on a miss                                        */
    int32_t *triangle;          /* index into that mesh's triangles as uploaded (rt_render_ids' numbering), -1 on a miss */
    float   *location;          /* [n][3] world location of the ACCEPTED hit (raycast.cu:98-102 for it); 0 on a miss     */
    float   *normal;            /* [n][3] world normal, raycast.cu:115-122; 0 on a miss                                  */
    float   *uv;                /* [n][2] interpolated texture uv, TrianglePrimitive::point_inside; 0 on a miss          */
    int32_t *pops;              /* [n] node pops of the cast (raycast.cu:61)                                             */
} RtRayHits;
size_t rt_trace_workspace_bytes(int32_t n);
int rt_trace_rays(RtScene *scene, const float *d_origins, const float *d_directions, int32_t n, const RtRayHits *out,
                  void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
/* Occlusion: cast_ray(ray, lighting_pass = true, light_distance = tmax[i]) with the early return of raycast.cu:129-133 restored
 * (the rule of the extension's shadow rays).  d_occluded[i] = 1 exactly when that cast accepts a hit at a distance below
 * tmax[i] -- i.e. when it returns min < tmax[i], except that a miss is not occluded when tmax[i] is +inf.  d_tmax NULL = FLT_MAX
 * for every ray. */
int rt_occluded(RtScene *scene, const float *d_origins, const float *d_directions, const float *d_tmax, int32_t n,
                uint8_t *d_occluded, void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
/* The primary ray of every pixel of a camera, exactly as the render kernels make it (raycast.cu:156-188, the fp64 island
 * included): DEVICE arrays [height * width][3], row-major (y * width + x); every origin is the camera position. */
int rt_camera_rays(const RtCameraParams *cam, float *d_origins, float *d_directions, void *stream, int synchronize);

/* ---- closest-point queries: the nearest point of the scene's triangles to each of the caller's points.
 *      The result equals a brute-force minimum over every (instance, triangle) bit for bit; it does not depend on the tree
 *      (host-built, device-built or refitted) nor on the order of traversal.  For world point p (fp32) and instance i:
 *      1. q = apply_lre(pose_i, p): the value the ray casts compute for an origin before the inv_scale multiply.  This "scaled
 *         mesh space" is world space rotated and translated, so distances there are world distances (any scale, mirrors too).
 *      2. Per triangle, the stored fp32 v0, e1 = v1 - v0, e0 = v2 - v0 scaled componentwise: A = v0*s, AB = e1*s, AC = e0*s.
 *         The closest point c = (A + b1*AB) + b2*AC per component, (b1, b2) from Ericson's region classification (Real-Time
 *         Collision Detection 5.1.5) over A, AB, AC, one fixed fp32 sequence without contraction.  An edge ratio whose
 *         denominator is not > 0 is 0, and none exceeds 1; the face weights are vb / sum and vc / sum.  Where the classification
 *         reaches the face region with va, vb or vc < 0 or sum <= 0 (nearly degenerate triangles, NaN), (b1, b2) is instead the
 *         nearest of the clamped projections onto the edges AB, AC, BC (first of equals in that order; a zero-length edge
 *         projects to its start).  So degenerate triangles never divide by zero and finite input gives a finite point.
 *      3. d2 = (dx*dx + dy*dy) + dz*dz in fp32 with d = q - c.
 *      4. A triangle is a candidate when d2 is not NaN and sqrtf(d2) <= max_distance[j] (inclusive; NULL = +inf).  A NaN or
 *         negative bound gives a miss (-0 counts as 0).  An overflowed d2 = +inf is a candidate under an infinite bound only.
 *      5. The winner is the candidate with the smallest (d2, instance index, triangle index), compared in that order; the
 *         triangle index is the caller's (rt_render_ids' and rt_trace_rays' numbering).
 *      Points are a DEVICE array [n][3]; outputs are optional tight DEVICE arrays indexed like the points.  Points with a
 *      non-finite component do not fault and do not change other points' results; their own results are unspecified.
 *      Asynchronous on `stream` unless synchronize != 0; nothing is launched when n == 0.  No scene scratch is used: calls may
 *      overlap each other and renders on other streams; a scene change on another stream is not ordered against them.
 *      RT_E_INVALID: NULL scene, n < 0, NULL points or no output at all with n > 0. ------------------------------------------- */
typedef struct RtPointHits {    /* every pointer optional (NULL = not wanted) */
    float   *distance;          /* sqrtf(d2) of the winner; FLT_MAX on a miss                                           */
    int32_t *instance;          /* the winner's instance index, -1 on a miss                                            */
    int32_t *triangle;          /* the winner's triangle index as uploaded (rt_render_ids' numbering), -1 on a miss     */
    float   *point;             /* [n][3] world position of c: apply_lre(inv_pose_i, c), raycast.cu:98-102's map; 0 on a miss */
    float   *normal;            /* [n][3] world face normal, as rt_trace_rays gives it; 0 on a miss                     */
    float   *barycentric;       /* [n][2] (b1, b2): the weights of v1 and v2; 0 on a miss                               */
    float   *uv;                /* [n][2] texture uv: w = (1 - b2) - b1, (w*uv0 + b1*uv1) + b2*uv2 per component; 0 on a miss */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the bit-exact contract)         */
} RtPointHits;
int rt_closest_points(RtScene *scene, const float *d_points, const float *d_max_distance, int32_t n, const RtPointHits *out,
                      void *stream, int synchronize);

/* ---- ray crossing counts, winding numbers and signed distance.  Integer results equal a brute-force
 *      count over every (instance, triangle), whatever the tree (host-built, device-built or refitted) and the order of traversal.
 *      For a ray (o, d), world fp32, and instance i:
 *      1. o' = apply_lre(pose_i, o), the map of rt_closest_points step 1; d' = apply_quat(q_pose_i, d), the direction rotated by
 *         the POSE quaternion.  (rt_trace_rays rotates d by the instance's `rotation` instead; the two agree for every instance
 *         made through the host API, whose rotation is the pose's ypr.  A C-ABI caller passing another rotation gets the
 *         geometry rt_closest_points sees.)
 *      2. The triangle A = v0*s, B = A + AB, C = A + AC, with A, AB, AC as in rt_closest_points step 2; the sums are fp32.
 *      3. The watertight ray/triangle test of Woop, Benthin and Wald (JCGT 2(1), 2013), one fixed fp32 sequence, no contraction:
 *         kz = the axis of the largest |d'| (first of equals in x, y, z order), kx = kz+1 mod 3, ky = kx+1 mod 3, kx and ky
 *         swapped when d'[kz] < 0.  Sx = d'[kx] / d'[kz], Sy = d'[ky] / d'[kz], Sz = 1 / d'[kz].  Per vertex P, p = P - o',
 *         px = p[kx] - Sx*p[kz], py = p[ky] - Sy*p[kz], pz = Sz*p[kz].  With a, b, c the vertices A, B, C:
 *         U = cx*by - cy*bx, V = ax*cy - ay*cx, W = bx*ay - by*ax; if any of U, V, W is 0, all three are recomputed in fp64
 *         from the same fp32 px, py and rounded to fp32, a nonzero value that rounds to 0 becoming +-2^-149 (the products are
 *         exact in fp64, so the signs are exact, and they survive the rounding).  A crossing
 *         needs (U, V, W all >= 0 or all <= 0; NaN fails both) and det = (U + V) + W != 0; then T = (U*az + V*bz) + W*cz and
 *         t = T / det.  The triangle is COUNTED when t > 0 and t <= tmax (NaN fails both).  Both faces count (rt_trace_rays
 *         never hits a back face).  A zero d' counts nothing.
 *      4. The sign of a counted triangle is +1 when det < 0, else -1: a ray LEAVING a closed mesh whose triangles are counter-
 *         clockwise seen from outside (the OBJ convention) counts +1, one entering it -1.  A mirrored instance (an odd number of
 *         negative scale components) flips that, as it flips its world triangles.
 *      5. count = the number of counted (instance, triangle) pairs, winding = the sum of their signs.  tmax is a ray PARAMETER
 *         (not a Euclidean distance as in rt_occluded): with d = b - a and tmax = 1, count is the number of crossings of the
 *         segment ab.  d_tmax NULL = +inf.  Rays with a non-finite component do not fault and do not change other rays'
 *         results; their own results are unspecified.
 *      6. The winding number of a point is the MEDIAN of its windings along RT_WINDING_D1..D3 (world directions, tmax = +inf).
 *         Triangles are stored as v0 and edge vectors, so B = A + AB can differ by rounding from the neighbouring triangle's
 *         vertex (always so with s != 1): a ray through such a shared edge can leak or count twice.  The test is not watertight
 *         across shared edges; the median of three fixed directions makes a wrong point need two unlucky rays.  Inside is
 *         winding != 0 (the nonzero rule); overlapping instances add up; a mirrored instance gives -1 inside.
 *      7. sdf = winding != 0 ? -distance : distance (fp32), distance exactly rt_closest_points' for the same point and
 *         max_distance, so -0.0 (a point on the surface counted inside) and -FLT_MAX (inside, no triangle within max_distance)
 *         occur.  The sign follows rule 6, not the nearest triangle's normal (normals give wrong signs at edges and vertices).
 *      Inputs are DEVICE arrays [n][3] (tmax / max_distance [n]); outputs are optional tight DEVICE arrays indexed like them.
 *      Asynchronous on `stream` unless synchronize != 0; nothing is launched when n == 0.  No workspace and no scene scratch: calls
 *      may overlap each other and renders on other streams; a scene change on another stream is not ordered against them.
 *      RT_E_INVALID: NULL scene, n < 0, NULL inputs or no output with n > 0. ---------------------------------------------------- */
#define RT_WINDING_D1 { 0x1.24b5dcp-1f, 0x1.3e5c92p-2f, 0x1.84c2f8p-1f }    /* ( 0.5717, 0.3109,  0.7593) */
#define RT_WINDING_D2 { -0x1.3f212ep-1f, 0x1.6d9e84p-1f, 0x1.46594ap-2f }   /* (-0.6233, 0.7141,  0.3187) */
#define RT_WINDING_D3 { 0x1.2809d4p-2f, 0x1.488ce8p-1f, -0x1.6bac72p-1f }   /* ( 0.2891, 0.6417, -0.7103) */
typedef struct RtCrossings {    /* every pointer optional (NULL = not wanted) */
    int32_t *count;             /* [n] counted (instance, triangle) pairs                                              */
    int32_t *winding;           /* [n] the sum of their signs                                                          */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the exact contract)            */
} RtCrossings;
int rt_count_crossings(RtScene *scene, const float *d_origins, const float *d_directions, const float *d_tmax, int32_t n,
                       const RtCrossings *out, void *stream, int synchronize);
int rt_winding_numbers(RtScene *scene, const float *d_points, int32_t n, int32_t *d_winding, void *stream, int synchronize);
/* d_sdf required; d_winding optional (the median winding of rule 6).  Runs rt_closest_points' kernel, then the winding kernel, on
 * `stream`. */
int rt_signed_distance(RtScene *scene, const float *d_points, const float *d_max_distance, int32_t n, float *d_sdf,
                       int32_t *d_winding, void *stream, int synchronize);

/* ---- crossing lists: every counted (instance, triangle) pair of a ray, sorted.
 *      8. The pairs of a ray are exactly those rules 1-5 count for rt_count_crossings (same tmax, d_tmax NULL = +inf).  Per pair:
 *         t = T / det of rule 3 in fp32 (a ray PARAMETER, the value compared with tmax); instance; triangle (the uploaded
 *         numbering of rt_render_ids / rt_trace_rays / rt_closest_points); sign (+-1, rule 4); barycentric (b1, b2) = the weights of
 *         v1 and v2 (rt_closest_points' convention), b1 = V / det and b2 = W / det in fp32 from the U, V, W the test used (after the
 *         fp64 fallback); uv: w = (1 - b2) - b1, then (w*uv0 + b1*uv1) + b2*uv2 per component (rt_closest_points' order and uv
 *         source); point: o_k + t*d_k per component in fp32, the WORLD point (scaled mesh space is world space rotated and
 *         translated, so a mesh-space t is a world parameter too).
 *         ORDER: a ray's pairs sorted by (t, instance, triangle) ascending.  A counted t is never NaN and is > 0, so the order is
 *         total and the list depends neither on the tree nor on the traversal.  Ties at one t are real (a shared edge, coincident
 *         triangles, overlapping instances).
 *         ROOMS: ray i owns the slots [start_i, start_i + room_i) of every output field and gets the first min(count_i, room_i)
 *         pairs of its sorted list.  The slots after those are padding: t = +inf, instance = triangle = -1, sign = 0, the float
 *         fields 0.  Nothing is ever written outside a ray's room, for any input (non-finite rays included, whose own contents are
 *         unspecified).  CSR: d_offsets int64 [n + 1], room_i = offsets[i+1] - offsets[i] (0 or less writes nothing), start_i =
 *         offsets[i].  Fixed: d_offsets NULL and max_hits = K >= 1, start_i = i*K (size_t), room_i = K (K = 1: the nearest crossing
 *         of either face, with exact barycentrics).
 *      rt_crossing_offsets writes offsets[0] = 0 and offsets[i+1] = offsets[i] + count_i (offsets[n] is the total; int64, so totals
 *      above 2^31 cannot overflow): the count traversal into the workspace, then an exclusive scan on the device.  Its workspace is
 *      DEVICE memory of at least rt_crossing_offsets_workspace_bytes(n) bytes (0 for n <= 0).  With n == 0 nothing is launched and
 *      d_offsets is not written.
 *      rt_list_crossings fills the rooms.  Every field of RtCrossingList is optional, at least one must be given; count[n] is each
 *      ray's FULL count, equal to rt_count_crossings' even when the room truncated the list (how a caller detects truncation).
 *      Given t, instance and triangle, one traversal inserts each pair into the sorted room; without one of them the room cannot
 *      hold the keys, and the kernel makes one traversal per filled slot instead (same result, slower).
 *      Both calls: inputs as for rt_count_crossings; asynchronous on `stream` unless synchronize != 0; no host synchronisation,
 *      allocation or copy to the host; no scene scratch (calls may overlap each other and renders); nothing launched when n == 0.
 *      RT_E_INVALID: the cases of rt_count_crossings; rt_crossing_offsets: d_offsets or d_workspace NULL, or a workspace too small,
 *      with n > 0; rt_list_crossings: both or neither of d_offsets and max_hits >= 1, no output field with n > 0. ------------- */
typedef struct RtCrossingList { /* every pointer optional (NULL = not wanted), at least one given; fields indexed by room slot */
    float *t;                   /* [slots]                                                                              */
    int32_t *instance;          /* [slots]                                                                              */
    int32_t *triangle;          /* [slots]                                                                              */
    int8_t *sign;               /* [slots] +1 / -1, 0 = padding                                                         */
    float *barycentric;         /* [slots][2] (b1, b2)                                                                  */
    float *uv;                  /* [slots][2]                                                                           */
    float *point;               /* [slots][3] world                                                                     */
    int32_t *count;             /* [n] the full count of each ray                                                       */
} RtCrossingList;
size_t rt_crossing_offsets_workspace_bytes(int32_t n);
int rt_crossing_offsets(RtScene *scene, const float *d_origins, const float *d_directions, const float *d_tmax, int32_t n,
                        int64_t *d_offsets, void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
int rt_list_crossings(RtScene *scene, const float *d_origins, const float *d_directions, const float *d_tmax, int32_t n,
                      const int64_t *d_offsets, int32_t max_hits, const RtCrossingList *out, void *stream, int synchronize);

/* ---- nearby-triangle lists: every (instance, triangle) within a radius of a point, sorted; k nearest.
 *      9. The pairs of point j are every (instance, triangle) whose d2, computed by rules 1-3 of rt_closest_points exactly, is a
 *         candidate under rule 4 with bound max_distance[j] (d_max_distance NULL = +inf; inclusive; a NaN or negative bound gives
 *         no pairs; a NaN d2 is never a pair; an overflowed d2 = +inf is a pair under an infinite bound only).
 *         ORDER: a point's pairs sorted by (d2, instance, triangle) ascending, rule 5's key, so slot 0 is rt_closest_points' winner.
 *         Per slot: distance = sqrtf(d2); instance; triangle (the uploaded numbering); point, normal, barycentric and uv each
 *         exactly as rt_closest_points computes them for that triangle.  The list depends neither on the tree (host-built,
 *         device-built or refitted) nor on the order of traversal.
 *         ROOMS: those of rule 8.  Point i owns the slots [start_i, start_i + room_i) of every output field and gets the first
 *         min(count_i, room_i) pairs of its sorted list; the slots after those are padding: distance = FLT_MAX, instance = triangle
 *         = -1, the other floats 0 (a closest-point miss).  Nothing is ever written outside a point's room, for any input
 *         (non-finite points and bounds included, whose own contents are unspecified).  CSR: d_offsets int64 [n + 1], room_i =
 *         offsets[i+1] - offsets[i] (0 or less writes nothing), start_i = offsets[i].  Fixed: d_offsets NULL and max_hits = K >= 1,
 *         start_i = i*K (size_t), room_i = K (K nearest within the bound; K = 1: rt_closest_points' winner).
 *      rt_nearby_offsets writes offsets[0] = 0 and offsets[i+1] = offsets[i] + count_i (int64): the count traversal into the
 *      workspace, then rt_crossing_offsets' exclusive scan on the device.  Its workspace is DEVICE memory of at least
 *      rt_nearby_offsets_workspace_bytes(n) bytes (0 for n <= 0).  With n == 0 nothing is launched and d_offsets is not written.
 *      rt_list_nearby fills the rooms.  distance, instance and triangle are REQUIRED (the room is where the keys live); the other
 *      fields are optional.  count[n] is each point's FULL number of pairs; pops[n] the interior nodes visited (a statistic, not
 *      part of the bit-exact contract).  In fixed rooms without count, the traversal prunes by the room's last key once the room
 *      is full (k-nearest); the rooms are the same bits with and without count.
 *      Both calls: inputs as for rt_closest_points; asynchronous on `stream` unless synchronize != 0; no host synchronisation,
 *      allocation or copy to the host; no scene scratch; nothing launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL points with n > 0; rt_nearby_offsets: d_offsets or d_workspace NULL, or a workspace too
 *      small, with n > 0; rt_list_nearby: NULL out, or distance, instance or triangle NULL, with n > 0; both or neither of
 *      d_offsets and max_hits >= 1. ----------------------------------------------------------------------------------------- */
typedef struct RtNearbyList {   /* fields indexed by room slot; distance, instance and triangle REQUIRED, the rest optional     */
    float *distance;            /* [slots] sqrtf(d2); FLT_MAX = padding                                                  */
    int32_t *instance;          /* [slots] -1 = padding                                                                  */
    int32_t *triangle;          /* [slots] the uploaded numbering; -1 = padding                                          */
    float *point;               /* [slots][3] world position of the triangle's closest point                             */
    float *normal;              /* [slots][3] world face normal                                                          */
    float *barycentric;         /* [slots][2] (b1, b2): the weights of v1 and v2                                         */
    float *uv;                  /* [slots][2] texture uv                                                                 */
    int32_t *count;             /* [n] the full number of pairs of each point                                            */
    int32_t *pops;              /* [n] interior nodes visited (a statistic)                                              */
} RtNearbyList;
size_t rt_nearby_offsets_workspace_bytes(int32_t n);
int rt_nearby_offsets(RtScene *scene, const float *d_points, const float *d_max_distance, int32_t n, int64_t *d_offsets,
                      void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
int rt_list_nearby(RtScene *scene, const float *d_points, const float *d_max_distance, int32_t n, const int64_t *d_offsets,
                   int32_t max_hits, const RtNearbyList *out, void *stream, int synchronize);

/* ---- triangle intersections: every (instance, triangle) of the scene that a caller's world triangle meets --
 *      collision and interference checks.  The pairs equal a brute-force loop over every (instance, triangle), whatever the tree.
 *      10. For query triangle j with world vertices P0, P1, P2 (fp32) and instance i:
 *          1. Query vertices: Qk = apply_lre(pose_i, Pk), rule 1's map into scaled mesh space.  The query triangle is (Q0, Q1, Q2).
 *          2. Scene triangle: A = v0*s, B = A + AB, C = A + AC, the fp32 sums of rule 2 (rt_closest_points' A, AB, AC).
 *          3. Box pre-test: per axis lo = fminf(fminf(x0, x1), x2) and hi = fmaxf(fmaxf(x0, x1), x2) over each triangle's three
 *             vertices; the pair passes when loT <= hiQ && loQ <= hiT on all three axes (NaN fails).
 *          4. Six segment tests in a fixed order: the query's edges Q0->Q1, Q1->Q2, Q2->Q0 against the triangle (A, B, C), then the
 *             scene triangle's edges A->B, B->C, C->A against (Q0, Q1, Q2).  Segment X->Y has o' = X and d' = Y - X (fp32 per
 *             component).  Each test is rule 3 with tmax = 1 on the triangle given by its three vertices (no b = a + ab is
 *             recomputed): the shear, U, V, W, the fp64 fallback with +-2^-149, det != 0 and 0 < t <= 1.  A zero d' counts nothing;
 *             both faces count.
 *          5. (i, triangle) is a PAIR of query j when step 3 passes and at least one of the six tests counts.
 *          6. Per pair: instance and triangle (the uploaded numbering of rt_render_ids / rt_trace_rays / rt_closest_points); normal =
 *             the world face normal exactly as rt_closest_points gives it; segment = [2][3] world points of the first and the last
 *             counting test in step 4's order, each X + t*d' per component in fp32, mapped to world by apply_lre(inv_pose_i, .)
 *             (closest_points' map).  The two ends are equal when only one test counts.
 *          7. ORDER: a query's pairs sorted by (instance, triangle) ascending.  ROOMS, padding and "nothing is ever written outside a
 *             room" are rule 8's; padding is instance = triangle = -1, normal and segment 0.
 *          8. skip_instance (optional int32 [n]): per query one instance whose pairs are never reported (-1 = none).  Instance k's own
 *             world triangles with skip_instance = k ask "what does instance k touch?".
 *      COPLANAR triangles: every segment test then rests on rounding in the sheared coordinates, so coplanar overlap is not reliably
 *      reported.  Closed meshes that touch face to face typically still report a contact, through side faces whose edges end on the
 *      shared plane.
 *      SHARED vertices and edges: the tests are closed, so triangles that share a vertex or an edge normally report a pair.  This is
 *      why the query is not (yet) a self-intersection test.
 *      NON-FINITE input: query triangles with a non-finite coordinate do not fault, do not change other queries' results and never
 *      write outside their room; their own results are unspecified.
 *      rt_count_intersecting: count [n] (the number of pairs), any [n] (1 when there is one), pops [n] (interior nodes visited, a
 *      statistic); all optional, at least one given.  With any and without count the traversal ends at the first pair, across
 *      instances too (the cheap collision check).
 *      rt_intersecting_offsets writes offsets[0] = 0 and offsets[i+1] = offsets[i] + count_i (int64): the count traversal into the
 *      workspace, then rt_crossing_offsets' exclusive scan on the device.  Its workspace is DEVICE memory of at least
 *      rt_intersecting_offsets_workspace_bytes(n) bytes (0 for n <= 0).  With n == 0 nothing is launched and d_offsets is not written.
 *      rt_list_intersecting fills the rooms: CSR (d_offsets) or fixed (d_offsets NULL, max_hits = K >= 1), as in rule 8.  instance and
 *      triangle are REQUIRED (the room is where the keys live), the rest optional; count[n] is each query's FULL count.  In fixed
 *      rooms without count, once a room is full the traversal ends after the instance of the room's last key; the rooms are the same
 *      bits with and without count.
 *      All calls: d_triangles is a DEVICE array [n][3][3] of world vertices; asynchronous on `stream` unless synchronize != 0; no host
 *      synchronisation, allocation or scene scratch (calls may overlap each other and renders); nothing launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL triangles with n > 0; rt_count_intersecting: NULL out or no output with n > 0;
 *      rt_intersecting_offsets: d_offsets or d_workspace NULL, or a workspace too small, with n > 0; rt_list_intersecting: NULL out,
 *      or instance or triangle NULL, with n > 0; both or neither of d_offsets and max_hits >= 1. ------------------------------- */
typedef struct RtIntersectCounts {  /* every pointer optional, at least one given                                              */
    int32_t *count;             /* [n] the number of pairs                                                                 */
    uint8_t *any;               /* [n] 1 when the query has a pair                                                         */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the exact contract)                */
} RtIntersectCounts;
typedef struct RtIntersectList {    /* fields indexed by room slot; instance and triangle REQUIRED, the rest optional          */
    int32_t *instance;          /* [slots] -1 = padding                                                                    */
    int32_t *triangle;          /* [slots] the uploaded numbering; -1 = padding                                            */
    float *normal;              /* [slots][3] world face normal                                                            */
    float *segment;             /* [slots][2][3] world points of the first and the last counting segment test             */
    int32_t *count;             /* [n] the full number of pairs of each query                                              */
    int32_t *pops;              /* [n] interior nodes visited (a statistic)                                                */
} RtIntersectList;
int rt_count_intersecting(RtScene *scene, const float *d_triangles, const int32_t *d_skip_instance, int32_t n,
                          const RtIntersectCounts *out, void *stream, int synchronize);
size_t rt_intersecting_offsets_workspace_bytes(int32_t n);
int rt_intersecting_offsets(RtScene *scene, const float *d_triangles, const int32_t *d_skip_instance, int32_t n, int64_t *d_offsets,
                            void *d_workspace, size_t workspace_bytes, void *stream, int synchronize);
int rt_list_intersecting(RtScene *scene, const float *d_triangles, const int32_t *d_skip_instance, int32_t n, const int64_t *d_offsets,
                         int32_t max_hits, const RtIntersectList *out, void *stream, int synchronize);

/* ---- box queries: every (instance, triangle) of the scene that meets a caller's world axis-aligned box, and
 *      occupancy grids -- voxelisers, occupancy maps, culling by region.  The pairs equal a brute-force loop over every (instance,
 *      triangle), whatever the tree (host-built, device-built, refitted) and whatever the traversal order.
 *      11. For query box j with world lo[3], hi[3] (fp32) and instance i; every operation fp32 in one fixed sequence, no contraction:
 *          1. Valid box: lo[a] <= hi[a] on all three axes.  A NaN or an inverted axis gives no pairs; lo == hi on an axis is a valid
 *             flat box (so is a line and a point).
 *          2. Corners: Ck = apply_lre(pose_i, corner_k), k = 0..7, rule 1's map into scaled mesh space; corner k takes hi on axis a
 *             when bit a of k is set (bit 0 = x), else lo.  Rk = Ck - C0 per component (R0 = 0).  The box edges are Ex = R1, Ey = R2,
 *             Ez = R4.
 *          3. Scene triangle: A = v0*s, B = A + AB, C = A + AC as in rule 10 step 2.  TA = A - C0, TB = B - C0, TC = C - C0;
 *             F0 = B - A, F1 = C - B, F2 = A - C.
 *          4. Box pre-test: per axis loQ / hiQ are the fminf / fmaxf chain over C0..C7 in that order, loT / hiT over A, B, C as in
 *             rule 10 step 3; the pair passes when loT <= hiQ && loQ <= hiT on all three axes (NaN fails).
 *          5. Thirteen separating axes in this order: Ex, Ey, Ez; N = cross(F0, F1); cross(Em, Fn) for m = x, y, z (outer) and
 *             n = 0, 1, 2 (inner).  cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x), each product rounded, then
 *             subtracted.  The projection on axis a is p(X) = (a.x*X.x + a.y*X.y) + a.z*X.z.  The box interval is the min and max of
 *             p(R0..R7), the triangle interval of p(TA), p(TB), p(TC), taken with fminf / fmaxf chains in the order given.  An axis
 *             SEPARATES when maxT < minB or maxB < minT; a zero axis or a NaN never separates.
 *          6. (i, triangle) is a PAIR of query j when step 1 holds, step 4 passes and no axis of step 5 separates.
 *          7. ORDER: a query's pairs sorted by (instance, triangle) ascending.  ROOMS (CSR or fixed K), padding (instance = triangle
 *             = -1) and "nothing is ever written outside a room" are rule 8's.
 *          8. NON-FINITE boxes do not fault, do not change other queries' results and never write outside their room; their own
 *             results are unspecified.
 *      NOT PROMISED: the test is closed (touching counts) and decided in fp32: a box and a triangle nearer to each other than the
 *      rounding of their coordinates can go either way.  Subtracting C0 keeps that rounding at the size of the box, not at the size
 *      of the scene.  Under a pose that is not the identity the mapped corners carry the map's rounding, so "exactly on a face"
 *      is decided in mesh space.
 *      rt_count_in_boxes: count [n] (the number of pairs), any [n] (1 when there is one), pops [n] (interior nodes visited, a
 *      statistic); all optional, at least one given.  With any and without count the traversal ends at the first pair, across
 *      instances too.
 *      rt_box_offsets writes offsets[0] = 0 and offsets[i+1] = offsets[i] + count_i (int64): the count traversal into the workspace,
 *      then rt_crossing_offsets' exclusive scan on the device.  Its workspace is DEVICE memory of at least
 *      rt_box_offsets_workspace_bytes(n) bytes (0 for n <= 0).  With n == 0 nothing is launched and d_offsets is not written.
 *      rt_list_in_boxes fills the rooms: CSR (d_offsets) or fixed (d_offsets NULL, max_hits = K >= 1), as in rule 8.  instance and
 *      triangle are REQUIRED (the room is where the keys live); count[n] is each query's FULL count.  In fixed rooms without count,
 *      once a room is full the traversal ends after the instance of the room's last key; the rooms are the same bits with and without
 *      count.
 *      rt_occupancy_grid runs rt_count_in_boxes on the cells of a regular grid that the kernel makes itself (no box array): origin,
 *      spacing [3] and dims [3] = (nx, ny, nz) are HOST arrays read during the call.  Cell (ix, iy, iz) is the box lo[a] = origin[a] +
 *      (float)i_a*spacing[a], hi[a] = origin[a] + (float)(i_a + 1)*spacing[a] (the product rounded, then the sum), so neighbouring
 *      cells share their faces bit for bit.  d_occupied (uint8) and d_count (int32) are [nz][ny][nx], x fastest, each optional, at
 *      least one given; they are bit-equal to rt_count_in_boxes' any and count on those boxes, and occupied without count stops at the
 *      first pair.  A negative spacing makes every cell an inverted box: all zeros.  A dimension of 0 launches nothing.
 *      All calls: d_boxes is a DEVICE array [n][2][3], lo then hi; asynchronous on `stream` unless synchronize != 0; no host
 *      synchronisation, allocation or scene scratch (calls may overlap each other and renders); nothing launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL boxes with n > 0; rt_count_in_boxes: NULL out or no output with n > 0; rt_box_offsets:
 *      d_offsets or d_workspace NULL, or a workspace too small, with n > 0; rt_list_in_boxes: NULL out, or instance or triangle NULL,
 *      with n > 0; both or neither of d_offsets and max_hits >= 1; rt_occupancy_grid: NULL origin, spacing or dims, a negative
 *      dimension, a dimension above 2^24, more than INT32_MAX cells, no output with at least one cell. ------------------------- */
typedef struct RtBoxCounts {        /* every pointer optional, at least one given                                              */
    int32_t *count;             /* [n] the number of pairs                                                                 */
    uint8_t *any;               /* [n] 1 when the query has a pair                                                         */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the exact contract)                */
} RtBoxCounts;
typedef struct RtBoxList {          /* fields indexed by room slot; instance and triangle REQUIRED, the rest optional          */
    int32_t *instance;          /* [slots] -1 = padding                                                                    */
    int32_t *triangle;          /* [slots] the uploaded numbering; -1 = padding                                            */
    int32_t *count;             /* [n] the full number of pairs of each query                                              */
    int32_t *pops;              /* [n] interior nodes visited (a statistic)                                                */
} RtBoxList;
int rt_count_in_boxes(RtScene *scene, const float *d_boxes, int32_t n, const RtBoxCounts *out, void *stream, int synchronize);
size_t rt_box_offsets_workspace_bytes(int32_t n);
int rt_box_offsets(RtScene *scene, const float *d_boxes, int32_t n, int64_t *d_offsets, void *d_workspace, size_t workspace_bytes,
                   void *stream, int synchronize);
int rt_list_in_boxes(RtScene *scene, const float *d_boxes, int32_t n, const int64_t *d_offsets, int32_t max_hits, const RtBoxList *out,
                     void *stream, int synchronize);
int rt_occupancy_grid(RtScene *scene, const float *origin, const float *spacing, const int32_t *dims, uint8_t *d_occupied,
                      int32_t *d_count, void *stream, int synchronize);

/* ---- plane sections: every (instance, triangle) of the scene that a caller's world plane cuts, with the
 *      oriented segment of the cut -- slicing for layered manufacturing, contour lines, section views.  The pairs equal a brute-force
 *      loop over every (instance, triangle), whatever the tree (host-built, device-built, refitted) and whatever the traversal order.
 *      12. For query plane j through the world point P with the world normal N (fp32, N not normalised) and instance i; every
 *          operation fp32 in one fixed sequence, no contraction:
 *          1. Valid plane: at least one component of N compares != 0.  A zero normal has no pairs.
 *          2. Map: p' = apply_lre(pose_i, P), rule 1's map of points; n' = apply_quat(q_pose_i, N), rule 1's map of directions.  Scaled
 *             mesh space is world space rotated and translated, so heights are world heights times |N|.
 *          3. Scene triangle: A = v0*s, B = A + AB, C = A + AC as in rule 10 step 2.
 *          4. Heights: h(X) = (n'.x*(X.x - p'.x) + n'.y*(X.y - p'.y)) + n'.z*(X.z - p'.z): each difference rounded, each product
 *             rounded, then the two sums.  A vertex is ABOVE when h >= 0 (so -0 is above), BELOW when h < 0; a NaN height is neither.
 *          5. (i, triangle) is a PAIR of plane j when step 1 holds, all three heights are classified, and at least one vertex is ABOVE
 *             and at least one BELOW.  The rule is half-open: a triangle lying in the plane is no pair; one touching the plane from
 *             above is no pair; one touching it from below with a vertex or an edge is a pair, with a zero-length segment or the edge
 *             itself.  So a closed surface yields closed contours and no coincident face is reported twice.
 *          6. Segment: exactly two edges of the cycle A->B->C->A join a BELOW and an ABOVE vertex.  On such an edge with BELOW end X and
 *             ABOVE end Y the cut point is t = hX / (hX - hY), Q = X + t*(Y - X) per component in fp32, always computed from the BELOW
 *             vertex whatever direction the cycle runs the edge in.  End 0 is the cut point of the edge the cycle runs from ABOVE to
 *             BELOW, end 1 that of the edge it runs from BELOW to ABOVE: end 0 -> end 1 runs along cross(n', face normal).  For a closed
 *             mesh counter-clockwise seen from outside, a triangle's end 1 lies on the edge that holds its neighbour's end 0, and the
 *             outer contour runs counter-clockwise seen from the side N points to.  A mirrored instance reverses that, as it reverses
 *             its world triangles.  Both ends go to world by apply_lre(inv_pose_i, Q), closest_points' map.
 *             NOT PROMISED: that neighbours' shared cut points are equal bit for bit.  Triangles are stored as v0 and edge vectors, so a
 *             shared vertex can differ by rounding between two triangles (rule 6's remark): the points coincide to rounding.
 *          7. Per pair: instance and triangle (the uploaded numbering); segment [2][3] world; normal [3] = the world face normal exactly
 *             as rt_closest_points gives it.  ORDER: a plane's pairs sorted by (instance, triangle) ascending.  ROOMS (CSR or fixed K),
 *             padding (instance = triangle = -1, the floats 0) and "nothing is ever written outside a room" are rule 8's.
 *          8. NON-FINITE planes, and planes whose heights overflow fp32 on this scene, do not fault, do not change other queries'
 *             results and never write outside their room; their own results are unspecified.
 *      rt_count_sections: count [n] (the number of pairs), any [n] (1 when there is one), pops [n] (interior nodes visited, a
 *      statistic); all optional, at least one given.  With any and without count the traversal ends at the first pair, across
 *      instances too.
 *      rt_section_offsets writes offsets[0] = 0 and offsets[i+1] = offsets[i] + count_i (int64): the count traversal into the
 *      workspace, then rt_crossing_offsets' exclusive scan on the device.  Its workspace is DEVICE memory of at least
 *      rt_section_offsets_workspace_bytes(n) bytes (0 for n <= 0).  With n == 0 nothing is launched and d_offsets is not written.
 *      rt_list_sections fills the rooms: CSR (d_offsets) or fixed (d_offsets NULL, max_hits = K >= 1), as in rule 8.  instance and
 *      triangle are REQUIRED (the room is where the keys live), the rest optional; count[n] is each plane's FULL count even when the
 *      room truncates.  In fixed rooms without count, once a room is full the traversal ends after the instance of the room's greatest
 *      key; the rooms are the same bits with and without count.
 *      All calls: d_planes is a DEVICE array [n][2][3], point then normal; asynchronous on `stream` unless synchronize != 0; no host
 *      synchronisation, allocation or scene scratch (calls may overlap each other and renders); nothing launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL planes with n > 0; rt_count_sections: NULL out or no output with n > 0;
 *      rt_section_offsets: d_offsets or d_workspace NULL, or a workspace too small, with n > 0; rt_list_sections: NULL out, or instance
 *      or triangle NULL, with n > 0; both or neither of d_offsets and max_hits >= 1. ------------------------------------------- */
typedef struct RtSectionCounts {    /* every pointer optional, at least one given                                              */
    int32_t *count;             /* [n] the number of pairs                                                                 */
    uint8_t *any;               /* [n] 1 when the plane has a pair                                                         */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the exact contract)                */
} RtSectionCounts;
typedef struct RtSectionList {      /* fields indexed by room slot; instance and triangle REQUIRED, the rest optional          */
    int32_t *instance;          /* [slots] -1 = padding                                                                    */
    int32_t *triangle;          /* [slots] the uploaded numbering; -1 = padding                                            */
    float *segment;             /* [slots][2][3] world ends of the cut, end 0 then end 1                                   */
    float *normal;              /* [slots][3] world face normal                                                            */
    int32_t *count;             /* [n] the full number of pairs of each plane                                              */
    int32_t *pops;              /* [n] interior nodes visited (a statistic)                                                */
} RtSectionList;
int rt_count_sections(RtScene *scene, const float *d_planes, int32_t n, const RtSectionCounts *out, void *stream, int synchronize);
size_t rt_section_offsets_workspace_bytes(int32_t n);
int rt_section_offsets(RtScene *scene, const float *d_planes, int32_t n, int64_t *d_offsets, void *d_workspace, size_t workspace_bytes,
                       void *stream, int synchronize);
int rt_list_sections(RtScene *scene, const float *d_planes, int32_t n, const int64_t *d_offsets, int32_t max_hits, const RtSectionList *out,
                     void *stream, int synchronize);

/* ---- segment queries: the nearest point of the scene's triangles to each of the caller's SEGMENTS, and whether
 *      a capsule (a segment with a radius) touches anything -- clearance and collision for characters, robot links, cables, tool
 *      sweeps.  rt_closest_points' contract widened from a point to a segment: the result equals a brute-force loop over every
 *      (instance, triangle) bit for bit, whatever the tree (host-built, device-built, refitted) and whatever the traversal order.
 *      13. For query segment j with the world end points P0, P1 (fp32) and instance i; every operation fp32 in one fixed sequence, no
 *          contraction:
 *          1. Map: Q0 = apply_lre(pose_i, P0), Q1 = apply_lre(pose_i, P1), rule 1's map into scaled mesh space; D = Q1 - Q0 per
 *             component.
 *          2. Scene triangle: A, AB, AC of rule 2.  Its edges (E0, F) are, in this order, (A, AB), (A, AC), (A + AB, AC - AB): the
 *             edges and the edge vectors of rule 2's nearest-edge fallback (A + AB and AC - AB are fp32 sums per component).
 *          3. Five candidates (s, b1, b2) per triangle, in this order:
 *             (a) the end Q0: (b1, b2) = rule 2's weights for the point Q0, s = 0;
 *             (b) the end Q1: (b1, b2) = rule 2's weights for the point Q1, s = 1;
 *             (c-e) the segment against each edge: the closest pair (s, u) of step 4, with (b1, b2) = (u, 0), (0, u), (1 - u, u).
 *                   They are taken only when dot(D, D) > 0: a segment of zero length (or one whose squared length underflows) is a
 *                   point, its candidates are the ends alone, and (a) is then rt_closest_points' answer bit for bit.
 *             Every candidate has X = Q0 + s*D per component (the product rounded, then the sum), c = (A + b1*AB) + b2*AC (rule 2) and
 *             d2 = (dx*dx + dy*dy) + dz*dz with d = X - c (rule 3).  The triangle's candidate is the one with the smallest d2, the
 *             first of equals in the order above; a NaN d2 never wins over one that is not NaN.
 *          4. Segment against segment (Ericson, Real-Time Collision Detection 5.1.9).  r = Q0 - E0, a = dot(D, D), e = dot(F, F),
 *             f = dot(F, r), dot(x, y) = x.x*y.x + x.y*y.y + x.z*y.z summed left to right, clamp01(x) = x > 0 ? (x < 1 ? x : 1) : 0 (a
 *             NaN gives 0).
 *               Neither a > 0 nor e > 0: s = u = 0.
 *               Not a > 0: s = 0, u = clamp01(f / e).
 *               Otherwise c = dot(D, r).
 *                 Not e > 0: u = 0, s = clamp01(-c / a).
 *                 Otherwise b = dot(D, F), den = a*e - b*b, s = den > 0 ? clamp01((b*f - c*e) / den) : 0, u = (b*s + f) / e;
 *                   if !(u >= 0): u = 0, s = clamp01(-c / a);  else if u > 1: u = 1, s = clamp01((b - c) / a).
 *             So s and u lie in [0, 1] always.  (Step 3 never reaches the first two lines; they make the routine total.)
 *          5. A triangle is a candidate of the query under rule 4 on its d2, with bound max_distance[j], the capsule's radius
 *             (inclusive; d_max_distance NULL = +inf; a NaN or negative bound gives no candidate).  The winner is the candidate
 *             with the smallest (d2, instance, triangle), rule 5's key.
 *          6. PIERCING is not part of the minimum: a segment through the middle of a large triangle has all five candidates far away.
 *             It is answered by rules 1-5 of rt_count_crossings for the ray o = P0, d = P1 - P0 (fp32 per component, world),
 *             tmax = 1, unchanged:  crossings = that count;  clearance = crossings > 0 ? 0 : distance;  within = (a candidate
 *             exists) || crossings > 0.  The point fields always describe the winner of step 5; a caller who wants the pierce points
 *             calls rt_list_crossings.  Both halves are equal to brute force on their own.
 *          7. NON-FINITE segments do not fault and do not change other queries' results; their own results are unspecified.
 *      d_segments is a DEVICE array [n][2][3], P0 then P1 (a box array's shape); outputs are optional tight DEVICE arrays indexed like the
 *      segments.  The distance half (every field but crossings) is one traversal; when within and / or pops are the only fields it
 *      feeds, it ends at the first candidate, across instances too (pops is then at most the full traversal's).  The crossing half runs
 *      only when crossings, clearance or within is wanted: rt_count_crossings' traversal on the same stream, patching the three in place
 *      (for within alone, only on the segments that have no candidate).
 *      Asynchronous on `stream` unless synchronize != 0; no workspace, no scene scratch, no host synchronisation (calls may overlap each
 *      other and renders on other streams; a scene change on another stream is not ordered against them); nothing is launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL segments or no output at all with n > 0. ------------------------------------------- */
typedef struct RtSegmentHits {  /* every pointer optional (NULL = not wanted), at least one given */
    float   *distance;          /* [n] sqrtf(d2) of the winner; FLT_MAX on a miss                                            */
    int32_t *instance;          /* [n] the winner's instance index, -1 on a miss                                             */
    int32_t *triangle;          /* [n] the winner's triangle index as uploaded, -1 on a miss                                 */
    float   *parameter;         /* [n] the winner's s in [0, 1]: where on the segment its nearest point lies; 0 on a miss    */
    float   *segment_point;     /* [n][3] world position of X: apply_lre(inv_pose_i, X); 0 on a miss                         */
    float   *point;             /* [n][3] world position of c: apply_lre(inv_pose_i, c); 0 on a miss                         */
    float   *normal;            /* [n][3] world face normal, as rt_closest_points gives it; 0 on a miss                      */
    float   *barycentric;       /* [n][2] (b1, b2): the weights of v1 and v2; 0 on a miss                                    */
    float   *uv;                /* [n][2] texture uv, rt_closest_points' sequence; 0 on a miss                               */
    int32_t *crossings;         /* [n] triangles the segment crosses (step 6)                                                */
    float   *clearance;         /* [n] crossings > 0 ? 0 : distance                                                          */
    int32_t *within;            /* [n] 1 when a triangle lies within max_distance of the segment or the segment crosses one, else 0 */
    int32_t *pops;              /* [n] interior nodes visited by the distance half (a statistic, not part of the exact contract) */
} RtSegmentHits;
int rt_closest_to_segments(RtScene *scene, const float *d_segments, const float *d_max_distance, int32_t n, const RtSegmentHits *out,
                           void *stream, int synchronize);

/* ---- triangle distance queries: the nearest point of the scene's triangles to each of the caller's TRIANGLES,
 *      and whether it lies within a clearance -- is this tool, link or part within 2 mm of anything, and where.  rt_closest_to_segments'
 *      contract widened from a segment to a triangle: the result equals a brute-force loop over every (instance, triangle) bit for bit,
 *      whatever the tree (host-built, device-built, refitted) and whatever the traversal order.
 *      14. For query triangle j with the world vertices P0, P1, P2 (fp32) and instance i; every operation fp32 in one fixed sequence, no
 *          contraction:
 *          1. Map: Qk = apply_lre(pose_i, Pk), rule 1's map into scaled mesh space; QAB = Q1 - Q0, QAC = Q2 - Q0 per component.  From
 *             here on the query triangle is (Q0, QAB, QAC), the form a scene triangle has.  A point of it is X = (Q0 + q1*QAB) + q2*QAC
 *             per component (rule 2's combination, each product rounded, then each sum).  Its vertices AS COMPUTED are V0 = Q0,
 *             V1 = Q0 + QAB, V2 = Q0 + QAC (fp32 sums; V1 may differ from Q1 in the last bit).  Its edges (G0, D) are, in this order,
 *             (Q0, QAB), (Q0, QAC), (V1, QAC - QAB).
 *          2. Scene triangle: A, AB, AC of rule 2.  Its vertices are W0 = A, W1 = A + AB, W2 = A + AC (fp32 sums); its edges (E0, F)
 *             are rule 13's in rule 13's order: (A, AB), (A, AC), (A + AB, AC - AB).
 *          3. Fifteen candidates (q1, q2, b1, b2) per pair, in this order:
 *             (a) 0-2: each query vertex against the scene triangle: (b1, b2) = rule 2's weights for the point Vk on (A, AB, AC);
 *                 (q1, q2) = (0, 0), (1, 0), (0, 1).  The point that is projected is the point that is priced: Vk, not Qk.
 *             (b) 3-5: each scene vertex against the query triangle: (q1, q2) = rule 2's weights for the point Wk on (Q0, QAB, QAC);
 *                 (b1, b2) = (0, 0), (1, 0), (0, 1).  Taken only when dot(QAB, QAB) > 0 || dot(QAC, QAC) > 0.
 *             (c) 6-14: query edge m (outer loop) against scene edge k (inner loop): (s, u) = rule 13 step 4's closest pair of
 *                 (G0_m, D_m) and (E0_k, F_k), unchanged;  (q1, q2) = (s, 0), (0, s), (1 - s, s) for m = 0, 1, 2;  (b1, b2) = (u, 0),
 *                 (0, u), (1 - u, u) for k = 0, 1, 2.  Edge m is taken only when dot(D_m, D_m) > 0.
 *             Every candidate is priced the same way: X as in step 1, c = (A + b1*AB) + b2*AC (rule 2), d2 = (dx*dx + dy*dy) + dz*dz with
 *             d = X - c (rule 3).  The pair's candidate is the one with the smallest d2, the first of equals in the order above; a NaN
 *             d2 never replaces one that is not NaN.
 *             The guards give one property bit for bit: a query triangle whose three vertices are equal is a point (QAB = QAC = 0),
 *             its candidates are (a) alone, V0 = V1 = V2, candidate 0 wins every tie, and the answer is rt_closest_points' answer in
 *             every field the two share.  No bit equality with rt_closest_to_segments is promised for a triangle that degenerates to a
 *             segment (two equal vertices, or three on a line): its third edge runs the segment in reverse and its (b) candidates
 *             project onto a degenerate triangle, and either may undercut rule 13's five in the last bits.
 *          4. A pair is a candidate of the query under rule 4 on its d2, with bound max_distance[j] (inclusive; d_max_distance NULL =
 *             +inf; a NaN or negative bound gives no candidate).  The winner is the candidate with the smallest (d2, instance,
 *             triangle), rule 5's key.
 *          5. INTERSECTION is not part of the minimum: two triangles that cross have fifteen small but non-zero candidates (each is a
 *             rounded closest pair of a vertex and a face or of two edges; the distance is 0 between an edge and a face's interior).
 *             That half is rule 10 of rt_count_intersecting on the same triangles, unchanged:  intersections = that count;
 *             clearance = intersections > 0 ? 0 : distance;  within = (a candidate exists) || intersections > 0.  The point fields
 *             always describe the winner of step 4; a caller who wants the contact segments calls rt_list_intersecting.  Both
 *             halves are equal to brute force on their own.  COPLANAR OVERLAP, which rule 10 does not report reliably (a segment in
 *             a triangle's plane counts nothing), reaches distance 0 through the edge and vertex candidates of step 3 instead: an
 *             edge crossing an edge or a vertex on a face has d2 = 0 wherever the arithmetic is exact, and a few ulps otherwise.
 *          6. d_skip_instance: optional int32 [n], -1 = none, as in rule 10: that instance contributes to neither half.  An instance's
 *             own world triangles with skip_instance = k ask how close instance k is to everything else.
 *          7. NON-FINITE triangles do not fault and do not change other queries' results; their own results are unspecified.
 *      d_triangles is a DEVICE array [n][3][3]; outputs are optional tight DEVICE arrays indexed like the triangles.  The distance half
 *      (every field but intersections) is one traversal; when within and / or pops are the only fields it feeds, it ends at the first
 *      candidate, across instances too (pops is then at most the full traversal's).  The intersection half runs only when
 *      intersections, clearance or within is wanted: rt_count_intersecting's traversal on the same stream, patching the three in place
 *      (counting every pair when intersections is wanted, else ending at the first; for within alone, only on the triangles that have
 *      no candidate).  A large query triangle prunes little (the bound is a box against a box): subdivide it on the host.
 *      Asynchronous on `stream` unless synchronize != 0; no workspace, no scene scratch, no host synchronisation (calls may overlap each
 *      other and renders on other streams; a scene change on another stream is not ordered against them); nothing is launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL triangles or no output at all with n > 0. ------------------------------------------ */
typedef struct RtTriangleHits { /* every pointer optional (NULL = not wanted), at least one given */
    float   *distance;          /* [n] sqrtf(d2) of the winner; FLT_MAX on a miss                                            */
    int32_t *instance;          /* [n] the winner's instance index, -1 on a miss                                             */
    int32_t *triangle;          /* [n] the winner's triangle index as uploaded, -1 on a miss                                 */
    float   *query_barycentric; /* [n][2] (q1, q2): the weights of P1 and P2 at the query triangle's nearest point; 0 on a miss */
    float   *query_point;       /* [n][3] world position of X: apply_lre(inv_pose_i, X); 0 on a miss                         */
    float   *point;             /* [n][3] world position of c: apply_lre(inv_pose_i, c); 0 on a miss                         */
    float   *normal;            /* [n][3] world face normal of the scene triangle, as rt_closest_points gives it; 0 on a miss */
    float   *barycentric;       /* [n][2] (b1, b2): the weights of v1 and v2; 0 on a miss                                    */
    float   *uv;                /* [n][2] texture uv, rt_closest_points' sequence; 0 on a miss                               */
    int32_t *intersections;     /* [n] scene triangles the query triangle intersects (step 5: rt_count_intersecting's count) */
    float   *clearance;         /* [n] intersections > 0 ? 0 : distance                                                      */
    int32_t *within;            /* [n] 1 when a triangle lies within max_distance of the query or the query intersects one, else 0 */
    int32_t *pops;              /* [n] interior nodes visited by the distance half (a statistic, not part of the exact contract) */
} RtTriangleHits;
int rt_closest_to_triangles(RtScene *scene, const float *d_triangles, const float *d_max_distance, const int32_t *d_skip_instance,
                            int32_t n, const RtTriangleHits *out, void *stream, int synchronize);

/* ---- sphere sweeps: the FIRST CONTACT of a sphere of radius r whose centre moves from P0 to P1 -- how far a
 *      character, a camera boom, a robot link or a tool can go before it touches the scene, and where it touches.  The moving form
 *      of rt_closest_to_segments' capsule test: the result equals a brute-force loop over every (instance, triangle) bit for bit,
 *      whatever the tree (host-built, device-built, refitted) and whatever the traversal order.
 *      16. For query j with the world positions P0, P1 of the centre (fp32), the radius r = radius[j] and instance i; every operation
 *          fp32 in one fixed sequence, no contraction; dot and d2 = (x*x + y*y) + z*z as in rule 13.  The radius is inclusive; a NaN or
 *          negative radius gives no contact (-0 counts as 0).
 *          1. Map: Q0, Q1 and D = Q1 - Q0 by rule 13 step 1.  The map is rigid, so r and the path parameter s mean the same in every
 *             instance and results compare across instances.  a = dot(D, D), r2 = r*r.
 *             M = the largest of |Q0.x|, |Q0.y|, |Q0.z|, |Q1.x|, |Q1.y|, |Q1.z| (taken by compares from 0: a NaN is passed over);
 *             reach = (r + r*2^-20) + M*2^-20;  reach2 = reach*reach.
 *          2. Scene triangle: A, AB, AC of rule 2; its edges (E0, F) are rule 13's in rule 13's order, its vertices A, A + AB, A + AC
 *             (fp32 sums).  Eight candidate TIMES s per triangle, in this order; a candidate counts only when 0 <= s <= 1 by compares:
 *             (0) the start: s = 0.
 *             (1) the face: N = (AB.y*AC.z - AB.z*AC.y, AB.z*AC.x - AB.x*AC.z, AB.x*AC.y - AB.y*AC.x); m = the largest |N_k| (as M
 *                 above); only when m > 0: U = N / m per component, lu = sqrtf(d2(U)), h0 = dot(U, Q0 - A), vn = dot(U, D);
 *                 h0 >= 0: g = h0 - r*lu, v = -vn;  h0 < 0: g = -h0 - r*lu, v = vn;  (neither: no candidate);  only when v > 0: s = g / v.
 *                 (The centre reaches the plane offset by r on Q0's side, moving towards it.  U keeps the squares in range for
 *                 coordinates from 1e-10 to 1e10.)
 *             (2-4) the edges' lines: only when ff = dot(F, F) > 0: w = Q0 - E0, tD = dot(D, F) / ff, tw = dot(w, F) / ff,
 *                 D' = D - tD*F, w' = w - tw*F per component (the product rounded, then the difference), a' = dot(D', D'); only when
 *                 a' > 0: s_mid = -dot(w', D') / a', d'2 = d2(w' + s_mid*D'); only when d'2 <= r2: s = s_mid - sqrtf((r2 - d'2) / a').
 *             (5-7) the vertices V: only when a > 0: w = Q0 - V, s_mid = -dot(w, D) / a, d'2 = d2(w + s_mid*D); only when d'2 <= r2:
 *                 s = s_mid - sqrtf((r2 - d'2) / a).
 *             (1-7) are taken only when a > 0: a sweep of zero length (or one whose squared length underflows) has the start alone.
 *             The edge and vertex roots are the closest-approach form, not (-b - sqrt(b*b - a*c)) / a: s_mid is the parameter of the
 *             line's nearest point to the feature and d'2 the squared distance there from the difference vector itself, so nothing
 *             cancels when the sphere starts many radii away.  Nothing divides by a value that a compare has not shown to be > 0.
 *          3. Verification: every candidate time is priced as rule 13 prices a candidate: X = Q0 + s*D per component (the product
 *             rounded, then the sum), (b1, b2) = rule 2's weights for the point X, c = (A + b1*AB) + b2*AC, d2 = d2(X - c).  It is
 *             VALID when d2 <= reach2 (a NaN fails).  No feature-region test is needed: a face root whose contact lies off the
 *             triangle, or an edge root beyond the edge's ends, has the centre farther than r from the triangle and fails.  The
 *             triangle's candidate is the valid one with the smallest s, the first of equals in the order above.
 *          4. The winner is the triangle candidate with the smallest (s, d2, instance, triangle).  With s = 0 (a sphere that starts
 *             in contact) the second component makes it the nearest triangle to P0: wherever rt_closest_points(P0, max_distance = r)
 *             has a winner, the sweep reports time 0 with the same instance, triangle, barycentrics and point, bit for bit (the start
 *             candidate is rule 2 on Q0, and reach2 is never below rule 4's bound for r).
 *          5. NON-FINITE queries do not fault and do not change other queries' results; their own results are unspecified.
 *          NOT PROMISED: the contact is decided in fp32.  The sphere's true distance at the reported time differs from r by a few
 *          ulps of r + M (DESIGN.md section 22 has the measurement); a path that comes within that of a triangle without crossing
 *          into it may be reported either way.  The constants are the smallest that lost no contact in that measurement.
 *      d_segments is a DEVICE array [n][2][3], P0 then P1 (rt_closest_to_segments' shape); d_radius a DEVICE array [n], REQUIRED; outputs
 *      are optional tight DEVICE arrays indexed like the queries.  One traversal; when hit and / or pops are the only outputs it ends
 *      at the first valid candidate, across instances too (pops is then at most the full traversal's).  A long sweep past much
 *      geometry prunes little until its first contact is found (the bound is a box against a box): split it on the host.
 *      Asynchronous on `stream` unless synchronize != 0; no workspace, no scene scratch, no host synchronisation (calls may overlap each
 *      other and renders on other streams; a scene change on another stream is not ordered against them); nothing is launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, NULL segments, radius or out, or no output at all, with n > 0. --------------------------- */
typedef struct RtSweepHits {    /* every pointer optional (NULL = not wanted), at least one given */
    float   *time;              /* [n] the winner's s in [0, 1]: the centre stops at P0 + s*(P1 - P0); FLT_MAX on a miss         */
    float   *distance;          /* [n] sqrtf(d2) at contact (r - distance is the penetration when time == 0); FLT_MAX on a miss  */
    int32_t *instance;          /* [n] the winner's instance index, -1 on a miss                                             */
    int32_t *triangle;          /* [n] the winner's triangle index as uploaded, -1 on a miss                                 */
    float   *centre;            /* [n][3] world position of X: apply_lre(inv_pose_i, X), segment_point's sequence; 0 on a miss */
    float   *point;             /* [n][3] world contact point c: apply_lre(inv_pose_i, c); 0 on a miss                       */
    float   *normal;            /* [n][3] world face normal, as rt_closest_points gives it; 0 on a miss                      */
    float   *contact_normal;    /* [n][3] from point towards centre: (X - c) / sqrtf(d2) per component, rotated to world by
                                 *        inv_rotation_i; the face normal where d2 > 0 fails; 0 on a miss                    */
    float   *barycentric;       /* [n][2] (b1, b2): the weights of v1 and v2 at the contact point; 0 on a miss               */
    float   *uv;                /* [n][2] texture uv, rt_closest_points' sequence; 0 on a miss                               */
    int32_t *hit;               /* [n] 1 when the sphere touches anything on its way, else 0                                 */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the exact contract)                  */
} RtSweepHits;
int rt_sweep_spheres(RtScene *scene, const float *d_segments, const float *d_radius, int32_t n, const RtSweepHits *out, void *stream,
                     int synchronize);

/* ---- region queries: every (instance, triangle) of the scene that lies in or touches a caller's convex REGION,
 *      the intersection of K half-spaces -- a view frustum, a selection pyramid, an oriented box, a wedge, a slab between two planes --
 *      and whether the triangle lies wholly inside.  Selection, culling, "what is in this workspace or sensor cone", clipping to a
 *      section box.  The pairs equal a brute-force loop over every (instance, triangle), whatever the tree (host-built, device-built,
 *      refitted) and whatever the traversal order.
 *      15. For region j, the planes (P_k, N_k), k = 0..K-1, in world space (fp32, N_k not normalised, pointing INWARD: the inside of a
 *          plane is its ABOVE side) and instance i; K is one value per call, 1 <= K <= RT_REGION_MAX_PLANES; every operation fp32 in
 *          one fixed sequence, no contraction:
 *          1. Valid region: every N_k has at least one component that compares != 0.  Any other region has no pairs.
 *          2. Map: p'_k, n'_k by rule 12 step 2; the scene triangle A = v0*s, B = A + AB, C = A + AC by rule 10 step 2; the height
 *             h_k(X) by rule 12 step 4 with (p'_k, n'_k), and rule 12's classes: ABOVE when h >= 0 (so -0 is above), BELOW when
 *             h < 0, neither for a NaN.
 *          3. Pre-test: on every plane all three vertices have a class and not all three are BELOW; otherwise no pair.
 *          4. Wholly inside: all three vertices ABOVE on every plane: a PAIR with inside = 1.
 *          5. Otherwise the polygon V = (A, B, C) is clipped in scaled mesh space by the planes in the order k = 0..K-1.  With m
 *             vertices (m < 3 too) and g_i = h_k(V_i) by step 2's formula, i = 0..m-1 walks the edge V_i -> V_((i+1) mod m): V_i is
 *             emitted when g_i >= 0; when exactly one of g_i >= 0 and g_(i+1) >= 0 holds, the cut is emitted after it, computed from
 *             the end X that is not above towards the end Y that is, by rule 12 step 6's formula: t = hX / (hX - hY),
 *             Q = X + t*(Y - X) per component.  A polygon holds at most 3 + RT_REGION_MAX_PLANES = 11 vertices: one that would be
 *             the twelfth is not emitted (only inconsistent roundings on nearly collinear vertices get there; it cannot empty a
 *             polygon).  An empty polygon after some plane: no pair.  A non-empty polygon after the last plane: a PAIR with
 *             inside = 0.  (A plane that has every current vertex above reproduces the polygon, so skipping it gives the same bits.)
 *          6. Per pair: instance and triangle (the uploaded numbering), inside, normal [3] = the world face normal exactly as
 *             rt_closest_points gives it.  ORDER: a region's pairs sorted by (instance, triangle) ascending.  ROOMS (CSR or fixed
 *             max_hits), padding (instance = triangle = -1, inside = 0, the floats 0) and "nothing is ever written outside a room"
 *             are rule 8's.
 *          7. NON-FINITE regions, and regions whose heights overflow fp32 on this scene, follow rule 12 step 8: no fault, no effect on
 *             other queries, nothing written outside their room; their own results are unspecified.
 *          NOT PROMISED: the test is CLOSED (touching counts) and decided in fp32, so a triangle nearer to a face than the rounding of
 *          the heights can go either way.  Face k's decision is relative to P_k: a caller who wants tight rounding puts P_k on the
 *          region's face, not at the origin.  The clipped polygon is not an output.
 *      rt_count_in_regions: count [n] (the number of pairs), inside [n] (the number of pairs with inside = 1), any [n] (1 when there is
 *      a pair), pops [n] (interior nodes visited, a statistic); all optional, at least one given.  With any and with neither count nor
 *      inside the traversal ends at the first pair, across instances too.
 *      rt_region_offsets writes offsets[0] = 0 and offsets[i+1] = offsets[i] + count_i (int64): the count traversal into the
 *      workspace, then rt_crossing_offsets' exclusive scan on the device.  Its workspace is DEVICE memory of at least
 *      rt_region_offsets_workspace_bytes(n) bytes (0 for n <= 0).  With n == 0 nothing is launched and d_offsets is not written.
 *      rt_list_in_regions fills the rooms: CSR (d_offsets) or fixed (d_offsets NULL, max_hits >= 1), as in rule 8.  instance and
 *      triangle are REQUIRED (the room is where the keys live), the rest optional; count[n] is each region's FULL count even when the
 *      room truncates.  In fixed rooms without count, once a room is full the traversal ends after the instance of the room's greatest
 *      key; the rooms are the same bits with and without count.
 *      All calls: d_regions is a DEVICE array [n][planes_per_region][2][3], point then normal, like a plane array; asynchronous on
 *      `stream` unless synchronize != 0; no host synchronisation, allocation or scene scratch (calls may overlap each other and
 *      renders); nothing launched when n == 0.
 *      RT_E_INVALID: NULL scene, n < 0, planes_per_region outside 1..RT_REGION_MAX_PLANES, NULL regions with n > 0;
 *      rt_count_in_regions: NULL out or no output with n > 0; rt_region_offsets: d_offsets or d_workspace NULL, or a workspace too
 *      small, with n > 0; rt_list_in_regions: NULL out, or instance or triangle NULL, with n > 0; both or neither of d_offsets and
 *      max_hits >= 1. ------------------------------------------------------------------------------------------------------------ */
#define RT_REGION_MAX_PLANES 8
typedef struct RtRegionCounts {     /* every pointer optional, at least one given                                              */
    int32_t *count;             /* [n] the number of pairs                                                                 */
    int32_t *inside;            /* [n] the number of pairs that lie wholly inside the region                               */
    uint8_t *any;               /* [n] 1 when the region has a pair                                                        */
    int32_t *pops;              /* [n] interior nodes visited (a statistic, not part of the exact contract)                */
} RtRegionCounts;
typedef struct RtRegionList {       /* fields indexed by room slot; instance and triangle REQUIRED, the rest optional          */
    int32_t *instance;          /* [slots] -1 = padding                                                                    */
    int32_t *triangle;          /* [slots] the uploaded numbering; -1 = padding                                            */
    uint8_t *inside;            /* [slots] 1 when the triangle lies wholly inside the region                               */
    float *normal;              /* [slots][3] world face normal                                                            */
    int32_t *count;             /* [n] the full number of pairs of each region                                             */
    int32_t *pops;              /* [n] interior nodes visited (a statistic)                                                */
} RtRegionList;
int rt_count_in_regions(RtScene *scene, const float *d_regions, int32_t n, int32_t planes_per_region, const RtRegionCounts *out,
                        void *stream, int synchronize);
size_t rt_region_offsets_workspace_bytes(int32_t n);
int rt_region_offsets(RtScene *scene, const float *d_regions, int32_t n, int32_t planes_per_region, int64_t *d_offsets, void *d_workspace,
                      size_t workspace_bytes, void *stream, int synchronize);
int rt_list_in_regions(RtScene *scene, const float *d_regions, int32_t n, int32_t planes_per_region, const int64_t *d_offsets,
                       int32_t max_hits, const RtRegionList *out, void *stream, int synchronize);

/* ---- timing on the stream the kernels run on (hipEvent) ---------------------------------- */
typedef struct RtTimer RtTimer;
int rt_timer_create(RtTimer **t);
int rt_timer_start(RtTimer *t, void *stream);
int rt_timer_stop(RtTimer *t, void *stream);
int rt_timer_elapsed_ms(RtTimer *t, float *ms);   /* synchronises on the stop event */
int rt_timer_destroy(RtTimer *t);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
