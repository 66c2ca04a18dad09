// Sensor.h -- a sensor that is not the reference's pinhole camera (no counterpart in the reference): any ray pattern with one
// centre of projection -- a spinning lidar, an equirectangular panorama, a fisheye, a Brown-Conrady camera -- given as one
// camera-space direction per pixel (+y the optical axis, +x image right, +z image up: the frame after raycast.cu:182).  Owns an
// RtRayTable (rt_hip.h, "sensor frames") and renders G-buffer and colour frames of a Scene from it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "Scene.h"
#include "transforms.hpp"

struct RtGBuffer;
struct RtPointCloud;
struct RtRayTable;

class Sensor {
public:
    // dirs: HOST [height][width][3] floats, row-major; copied to the device and packed before the constructor returns.
    // A sensor that could not be made (a bad size, no memory, no device) has last_error != 0 and refuses every call.
    Sensor(const float* dirs, int width, int height);
    ~Sensor();
    Sensor(const Sensor&) = delete;
    Sensor& operator=(const Sensor&) = delete;

    transforms::lre pose;
    int width;
    int height;
    void* stream = nullptr;                        // hipStream_t
    int last_error = 0;

    void set_pose(const transforms::lre& p) { pose = p; }
    void set_stream(void* s) { stream = s; }
    const RtRayTable* table() const { return d_table; }
    // The rays of the current pose (rt_ray_table_rays): DEVICE origins and world directions [height * width][3].  Asynchronous on
    // `stream`; returns last_error.
    int rays(float* d_origins, float* d_directions);
    // G-buffer frames (rt_render_gbuffer_table in rt_hip.h): frame i is this sensor at poses[i]; `out` holds the wanted DEVICE planes,
    // frame-major; d_imgs null = no colour frames.  1..RT_MAX_BATCH poses per call.  Asynchronous on `stream`; returns last_error.
    int render_gbuffer(Scene& scene, const std::vector<transforms::lre>& poses, const RtGBuffer& out, uint8_t* const* d_imgs = nullptr,
                       size_t pitch = 0);
    // The same two with the pose and the stream as arguments: they read the sensor and write nothing in it, so any number of host
    // threads may call them on one sensor at once.  They return the error code and leave last_error alone.
    int rays_on(void* on_stream, const transforms::lre& at, float* d_origins, float* d_directions) const;
    int render_gbuffer_on(void* on_stream, Scene& scene, const std::vector<transforms::lre>& poses, const RtGBuffer& out,
                          uint8_t* const* d_imgs = nullptr, size_t pitch = 0) const;
    // Point cloud, first step (rt_point_cloud_offsets_table in rt_hip.h): as Camera::point_cloud_offsets, the rays from this
    // sensor's table.  Writes nothing in the sensor; returns the error code and leaves last_error alone.
    int point_cloud_offsets(void* on_stream, Scene& scene, const std::vector<transforms::lre>& poses, float min_range, float max_range,
                            const uint8_t* d_mask, uint32_t fields, int64_t* d_offsets, void* d_workspace, size_t workspace_bytes) const;
    // Rolling frames (rt_render_gbuffer_rolling in rt_hip.h): a pose per slice of slice_pixels columns (axis 0) or rows (axis 1).
    // poses: [count][slices] flattened, slices = rolling_slices(axis, slice_pixels); the inverse of each is the host's own invert_lre.
    // d_local: optional DEVICE plane [count][height][width][3]; d_workspace: rt_rolling_workspace_bytes(count, slices) DEVICE bytes.
    // Writes nothing in the sensor; returns the error code and leaves last_error alone.
    int rolling_slices(int axis, int slice_pixels) const;       // 0 for a bad axis or slice_pixels
    int render_rolling_on(void* on_stream, Scene& scene, const std::vector<transforms::lre>& poses, int count, int axis, int slice_pixels,
                          const RtGBuffer& out, float* d_local, void* d_workspace, size_t workspace_bytes, uint8_t* const* d_imgs = nullptr,
                          size_t pitch = 0) const;
    // Rolling cloud, first step (rt_point_cloud_offsets_rolling in rt_hip.h); the workspace is
    // rt_point_cloud_rolling_workspace_bytes(width, height, count, fields, slices) bytes.
    int point_cloud_offsets_rolling(void* on_stream, Scene& scene, const std::vector<transforms::lre>& poses, int count, int axis,
                                    int slice_pixels, float min_range, float max_range, const uint8_t* d_mask, uint32_t fields,
                                    int64_t* d_offsets, void* d_workspace, size_t workspace_bytes) const;

private:
    RtRayTable* d_table = nullptr;
};

// Point cloud, second step (rt_point_cloud_fill in rt_hip.h; also declared in Camera.h): the points of the workspace a
// point_cloud_offsets call of a camera or sensor of this size left, with the same poses and fields, into the wanted DEVICE arrays of
// `out`, the first `capacity` of them.  Needs no scene.  Asynchronous on `on_stream`; returns the error code.
int point_cloud_fill(void* on_stream, int width, int height, const std::vector<transforms::lre>& poses, uint32_t fields,
                     const void* d_workspace, size_t workspace_bytes, int64_t capacity, const RtPointCloud& out);
// Rolling cloud, second step (rt_point_cloud_fill_rolling in rt_hip.h): the points of the workspace a point_cloud_offsets_rolling
// call left, with the same size, count, axis, slice_pixels and fields.  Needs neither the scene nor the poses: the pose records are
// in the workspace.  Asynchronous on `on_stream`; returns the error code.
int point_cloud_fill_rolling(void* on_stream, int width, int height, int count, int axis, int slice_pixels, uint32_t fields,
                             const void* d_workspace, size_t workspace_bytes, int64_t capacity, const RtPointCloud& out);
