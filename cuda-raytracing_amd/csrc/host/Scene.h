// Scene.h -- the host scene graph: what was added, and the device copy made from it.
//
// Same calls as the reference's Scene (Scene.h:19-28): add_* store by value and hand back nothing (indices are the
// insertion order), upload_to_device() (re)builds the device scene, update_mesh_instance() re-poses one instance
// without rebuilding.  The device side is owned by librt_hip.so behind `d_scene` (an RtScene*, see include/rt_hip.h)
// instead of the reference's three raw device pointers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "Material.hpp"
#include "MeshInstance.hpp"
#include "MeshPrimitive.h"

struct RtScene;
struct RtRayHits;
struct RtPointHits;
struct RtCrossings;
struct RtCrossingList;
struct RtNearbyList;
struct RtIntersectCounts;
struct RtIntersectList;
struct RtBoxCounts;
struct RtBoxList;
struct RtSectionCounts;
struct RtSectionList;
struct RtSegmentHits;
struct RtTriangleHits;
struct RtSweepHits;
struct RtRegionCounts;
struct RtRegionList;
struct RtVisibility;

class Scene {
public:
    Scene();
    ~Scene();                                       // releases the device scene
    Scene(const Scene&) = delete;                   // owns device memory
    Scene& operator=(const Scene&) = delete;

    // ---- what the scene contains (host side) ----
    void add_mesh(MeshPrimitive mesh);
    void add_material(Material material);
    void add_mesh_instance(MeshInstance mesh_instance);
    int num_materials() const { return (int)materials.size(); }
    Material& material(int index) { return materials[index]; }      // edit before upload_to_device()

    // ---- device side ----
    void upload_to_device();                        // flatten everything and call rt_scene_upload (Scene.cpp:25-65)
    void update_mesh_instance(int index, MeshInstance mesh_instance);   // rt_scene_update_instance (Scene.cpp:67-74)
    // the same, ordered on a stream instead of synchronising (rt_scene_update_instance_async): for per-frame animation
    void update_mesh_instance(int index, MeshInstance mesh_instance, void* stream);
    // Direction tables of batched launches (rt_scene_dir_table_stats of include/rt_hip.h): launches that read one, view launches
    // that did not, buffer growths, bytes held.  Returns the status (also in last_error).
    int dir_table_stats(uint64_t out[4]);
    // Back-facing leaves culled in the views of the scene's last batched launch (rt_scene_view_cull_stats of include/rt_hip.h; it waits
    // for the device): *frames = the frames of that launch, 0 when its views hold no culled box; culled_leaves[k] for k < *frames, room
    // for 32 entries.  Returns the status (also in last_error).
    int view_cull_stats(int32_t* frames, uint64_t* culled_leaves);
    // A mesh deforms (same triangle count and order): host copy and device copy get the moved vertices and normals and refitted
    // bounds -- texture coordinates stay; no rebuild, no re-upload of anything else.  Ordered on `stream` like update_mesh_instance(.., stream).
    void refit_mesh(int mesh_index, std::vector<TrianglePrimitive> moved, void* stream = nullptr);
    // A mesh changes beyond what a refit can follow (large motion, or other triangles): the device copy gets a NEW tree, built on
    // the GPU straight into the scene's arrays (rt_scene_rebuild_mesh_device), the host copy rebuilds its tree when it is next
    // needed.  More triangles than the mesh was uploaded with do not fit its part of the arrays: a new device scene is uploaded
    // then (the GPU builds the mesh's tree during the upload) and takes the old one's place once it is complete; that path waits
    // for the whole device, whatever `stream` is.  On EVERY path the host mesh and the device scene change only after the device
    // call has succeeded: on an error (last_error) host and device still describe the old mesh and the old scene still renders.
    // Returns when the new tree is in place.
    void rebuild_mesh(int mesh_index, std::vector<TrianglePrimitive> triangles, void* stream = nullptr);
    // Ray queries on the device scene: the reference's cast_ray (raycast.cu:21-142) on rays the caller chooses -- rt_trace_rays /
    // rt_occluded of include/rt_hip.h, where the semantics are.  Rays and outputs are DEVICE arrays; a workspace of
    // rt_trace_workspace_bytes(n) bytes (optional) sorts the rays by direction octant first.  Returns the status (also in last_error).
    int trace_rays(const float* d_origins, const float* d_directions, int32_t n, const RtRayHits& out, void* d_workspace = nullptr,
                   size_t workspace_bytes = 0, void* stream = nullptr, bool synchronize = false);
    int occluded(const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, uint8_t* d_occluded,
                 void* d_workspace = nullptr, size_t workspace_bytes = 0, void* stream = nullptr, bool synchronize = false);
    // Closest-point queries on the device scene: rt_closest_points of include/rt_hip.h, where the semantics are.  Points, bounds
    // (optional, NULL = +inf) and outputs are DEVICE arrays.  Returns the status (also in last_error).
    int closest_points(const float* d_points, const float* d_max_distance, int32_t n, const RtPointHits& out, void* stream = nullptr,
                       bool synchronize = false);
    // Crossing counts, winding numbers and signed distance on the device scene: rt_count_crossings / rt_winding_numbers /
    // rt_signed_distance of include/rt_hip.h, where the semantics are.  Inputs and outputs are DEVICE arrays.  Return the status.
    int count_crossings(const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, const RtCrossings& out,
                        void* stream = nullptr, bool synchronize = false);
    int winding_numbers(const float* d_points, int32_t n, int32_t* d_winding, void* stream = nullptr, bool synchronize = false);
    int signed_distance(const float* d_points, const float* d_max_distance, int32_t n, float* d_sdf, int32_t* d_winding = nullptr,
                        void* stream = nullptr, bool synchronize = false);
    // Crossing lists on the device scene: rt_crossing_offsets / rt_list_crossings of include/rt_hip.h (rule 8, rooms), where the
    // semantics are.  Inputs, offsets, workspace and outputs are DEVICE arrays.  Return the status.
    int crossing_offsets(const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, int64_t* d_offsets,
                         void* d_workspace, size_t workspace_bytes, void* stream = nullptr, bool synchronize = false);
    int list_crossings(const float* d_origins, const float* d_directions, const float* d_tmax, int32_t n, const int64_t* d_offsets,
                       int32_t max_hits, const RtCrossingList& out, void* stream = nullptr, bool synchronize = false);
    // Nearby-triangle lists on the device scene: rt_nearby_offsets / rt_list_nearby of include/rt_hip.h (rule 9, rooms), where the
    // semantics are.  Inputs, offsets, workspace and outputs are DEVICE arrays.  Return the status.
    int nearby_offsets(const float* d_points, const float* d_max_distance, int32_t n, int64_t* d_offsets, void* d_workspace,
                       size_t workspace_bytes, void* stream = nullptr, bool synchronize = false);
    int list_nearby(const float* d_points, const float* d_max_distance, int32_t n, const int64_t* d_offsets, int32_t max_hits,
                    const RtNearbyList& out, void* stream = nullptr, bool synchronize = false);
    // Triangle intersections on the device scene: rt_count_intersecting / rt_intersecting_offsets / rt_list_intersecting of
    // include/rt_hip.h (rule 10, rooms), where the semantics are.  Triangles ([n][3][3] world), skip_instance (optional), offsets,
    // workspace and outputs are DEVICE arrays.  Return the status.
    int count_intersecting(const float* d_triangles, const int32_t* d_skip_instance, int32_t n, const RtIntersectCounts& out,
                           void* stream = nullptr, bool synchronize = false);
    int intersecting_offsets(const float* d_triangles, const int32_t* d_skip_instance, int32_t n, int64_t* d_offsets, void* d_workspace,
                             size_t workspace_bytes, void* stream = nullptr, bool synchronize = false);
    int list_intersecting(const float* d_triangles, const int32_t* d_skip_instance, int32_t n, const int64_t* d_offsets, int32_t max_hits,
                          const RtIntersectList& out, void* stream = nullptr, bool synchronize = false);
    // Box queries on the device scene: rt_count_in_boxes / rt_box_offsets / rt_list_in_boxes / rt_occupancy_grid of include/rt_hip.h
    // (rule 11, rooms), where the semantics are.  Boxes ([n][2][3] world, lo then hi), offsets, workspace and outputs are DEVICE
    // arrays; origin, spacing and dims of the grid are host arrays of 3.  Return the status.
    int count_in_boxes(const float* d_boxes, int32_t n, const RtBoxCounts& out, void* stream = nullptr, bool synchronize = false);
    int box_offsets(const float* d_boxes, int32_t n, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes,
                    void* stream = nullptr, bool synchronize = false);
    int list_in_boxes(const float* d_boxes, int32_t n, const int64_t* d_offsets, int32_t max_hits, const RtBoxList& out,
                      void* stream = nullptr, bool synchronize = false);
    int occupancy_grid(const float* origin, const float* spacing, const int32_t* dims, uint8_t* d_occupied, int32_t* d_count,
                       void* stream = nullptr, bool synchronize = false);
    // Plane sections on the device scene: rt_count_sections / rt_section_offsets / rt_list_sections of include/rt_hip.h (rule 12,
    // rooms), where the semantics are.  Planes ([n][2][3] world, point then normal), offsets, workspace and outputs are DEVICE
    // arrays.  Return the status.
    int count_sections(const float* d_planes, int32_t n, const RtSectionCounts& out, void* stream = nullptr, bool synchronize = false);
    int section_offsets(const float* d_planes, int32_t n, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes,
                        void* stream = nullptr, bool synchronize = false);
    int list_sections(const float* d_planes, int32_t n, const int64_t* d_offsets, int32_t max_hits, const RtSectionList& out,
                      void* stream = nullptr, bool synchronize = false);
    // Segment queries on the device scene: rt_closest_to_segments of include/rt_hip.h (rule 13), where the semantics are.  Segments
    // ([n][2][3] world, P0 then P1), radii (optional, NULL = +inf) and outputs are DEVICE arrays.  Returns the status.
    int closest_to_segments(const float* d_segments, const float* d_max_distance, int32_t n, const RtSegmentHits& out,
                            void* stream = nullptr, bool synchronize = false);
    // Triangle distance queries on the device scene: rt_closest_to_triangles of include/rt_hip.h (rule 14), where the semantics are.
    // Triangles ([n][3][3] world), radii and skipped instances (both optional, NULL = +inf / none) and outputs are DEVICE arrays.
    // Returns the status.
    int closest_to_triangles(const float* d_triangles, const float* d_max_distance, const int32_t* d_skip_instance, int32_t n,
                             const RtTriangleHits& out, void* stream = nullptr, bool synchronize = false);
    // Sphere sweeps on the device scene: rt_sweep_spheres of include/rt_hip.h (rule 16), where the semantics are.  Segments
    // ([n][2][3] world, the centre's P0 then P1), radii ([n], required) and outputs are DEVICE arrays.  Returns the status.
    int sweep_spheres(const float* d_segments, const float* d_radius, int32_t n, const RtSweepHits& out, void* stream = nullptr,
                      bool synchronize = false);
    // Region queries on the device scene: rt_count_in_regions / rt_region_offsets / rt_list_in_regions of include/rt_hip.h (rule 15,
    // rooms), where the semantics are.  Regions ([n][planes_per_region][2][3] world, point then inward normal), offsets, workspace
    // and outputs are DEVICE arrays.  Return the status.
    int count_in_regions(const float* d_regions, int32_t n, int32_t planes_per_region, const RtRegionCounts& out, void* stream = nullptr,
                         bool synchronize = false);
    int region_offsets(const float* d_regions, int32_t n, int32_t planes_per_region, int64_t* d_offsets, void* d_workspace,
                       size_t workspace_bytes, void* stream = nullptr, bool synchronize = false);
    int list_in_regions(const float* d_regions, int32_t n, int32_t planes_per_region, const int64_t* d_offsets, int32_t max_hits,
                        const RtRegionList& out, void* stream = nullptr, bool synchronize = false);
    // Visibility masks on the device scene: rt_visibility of include/rt_hip.h ("visibility masks"), where the rule is.  The planes
    // ([count][height][width](x3), a G-buffer's instance, location and -- for `facing` -- normal), the points ([count][num_points][3]
    // world) and the masks are DEVICE arrays.  Returns the status.
    int visibility(const int32_t* d_instance, const float* d_location, const float* d_normal, int32_t width, int32_t height, int32_t count,
                   const float* d_points, int32_t num_points, float bias, const RtVisibility& out, void* stream = nullptr,
                   bool synchronize = false);
    RtScene* d_scene = nullptr;
    int num_mesh_instances = 0;
    int last_error = 0;                             // rt_hip.h status of the last device call (the reference ignores errors)

private:
    int upload_as(const std::vector<MeshPrimitive*>& meshes_now, RtScene** out);   // a new device scene from these meshes; touches nothing else
    std::vector<MeshPrimitive> meshes;
    std::vector<Material> materials;
    std::vector<MeshInstance> mesh_instances;
};
