"""The `stream` argument of the query wrappers on the torch path, in both forms the docstrings promise: a torch.cuda.Stream and the raw
hipStream_t of one.  Every query family (rays, points, crossings, nearby lists, triangle intersections, boxes and occupancy grids,
plane sections, regions, segments, triangle distances) runs once with each on a stream that is not the current one, and both results equal the numpy path's for the same inputs bit for
bit (the numpy path is held to the oracles by the family's own tests: none is needed here)."""
import numpy as np
import pytest

import scene_defs as sd

pytestmark = pytest.mark.gpu
F32 = np.float32
N = 65                                      # one full wave and one lane


def _queries(s, q, **kw):
    """name -> zero-argument call of every query family on the arrays of q (numpy or torch), list queries in CSR and fixed-room form"""
    o, d, tmax, pts, md, tris, skip = (q[k] for k in ("o", "d", "tmax", "pts", "md", "tris", "skip"))
    nearby = s.NEARBY_LIST_OUTPUTS + ("count", "pops")
    pairs = s.INTERSECT_LIST_OUTPUTS + ("count", "pops")
    boxed = s.BOX_LIST_OUTPUTS + ("count", "pops")
    cut = s.SECTION_LIST_OUTPUTS + ("count", "pops")
    held = s.REGION_LIST_OUTPUTS + ("count", "pops")
    grid_kw = kw or dict(as_numpy=True)                         # (the grid takes no arrays: numpy results are asked for by name)
    return {
        "trace_rays": lambda: s.trace_rays(o, d, outputs=s.RAY_OUTPUTS, **kw),
        "occluded": lambda: {"occluded": s.occluded(o, d, tmax, binning=True, **kw)},
        "closest_points": lambda: s.closest_points(pts, md, outputs=s.POINT_OUTPUTS, **kw),
        "count_crossings": lambda: s.count_crossings(o, d, tmax, outputs=s.CROSSING_OUTPUTS, **kw),
        "winding_numbers": lambda: {"winding": s.winding_numbers(pts, **kw)},
        "signed_distance": lambda: {"sdf": s.signed_distance(pts, md, **kw)},
        "list_crossings_csr": lambda: s.list_crossings(o, d, tmax, **kw),
        "list_crossings_k2": lambda: s.list_crossings(o, d, tmax, max_hits=2, **kw),
        "list_nearby_csr": lambda: s.list_nearby(pts, md, outputs=nearby, **kw),
        "list_nearby_k2": lambda: s.list_nearby(pts, md, max_hits=2, outputs=nearby, **kw),
        "count_intersecting": lambda: s.count_intersecting(tris, skip, outputs=s.INTERSECT_COUNT_OUTPUTS, **kw),
        "list_intersecting_csr": lambda: s.list_intersecting(tris, skip, outputs=pairs, **kw),
        "list_intersecting_k2": lambda: s.list_intersecting(tris, skip, max_hits=2, outputs=pairs, **kw),
        "count_in_boxes": lambda: s.count_in_boxes(q["boxes"], outputs=s.BOX_COUNT_OUTPUTS, **kw),
        "list_in_boxes_csr": lambda: s.list_in_boxes(q["boxes"], outputs=boxed, **kw),
        "list_in_boxes_k2": lambda: s.list_in_boxes(q["boxes"], max_hits=2, outputs=boxed, **kw),
        "occupancy_grid": lambda: s.occupancy_grid(GRID[0], GRID[1], GRID[2], outputs=s.GRID_OUTPUTS, **grid_kw),
        "count_sections": lambda: s.count_sections(q["planes"], outputs=s.SECTION_COUNT_OUTPUTS, **kw),
        "list_sections_csr": lambda: s.list_sections(q["planes"], outputs=cut, **kw),
        "list_sections_k2": lambda: s.list_sections(q["planes"], max_hits=2, outputs=cut, **kw),
        "count_in_regions": lambda: s.count_in_regions(q["regions"], outputs=s.REGION_COUNT_OUTPUTS, **kw),
        "list_in_regions_csr": lambda: s.list_in_regions(q["regions"], outputs=held, **kw),
        "list_in_regions_k2": lambda: s.list_in_regions(q["regions"], max_hits=2, outputs=held, **kw),
        "closest_to_segments": lambda: s.closest_to_segments(q["segs"], md, outputs=s.SEGMENT_OUTPUTS, **kw),
        "closest_to_triangles": lambda: s.closest_to_triangles(tris, md, skip, outputs=s.TRIANGLE_HIT_OUTPUTS, **kw),
    }


QUERIES = ("trace_rays", "occluded", "closest_points", "count_crossings", "winding_numbers", "signed_distance", "list_crossings_csr",
           "list_crossings_k2", "list_nearby_csr", "list_nearby_k2", "count_intersecting", "list_intersecting_csr", "list_intersecting_k2",
           "count_in_boxes", "list_in_boxes_csr", "list_in_boxes_k2", "occupancy_grid", "count_sections", "list_sections_csr",
           "list_sections_k2", "count_in_regions", "list_in_regions_csr", "list_in_regions_k2", "closest_to_segments",
           "closest_to_triangles")
GRID = ((-1.3, -1.2, -1.1), (0.41, 0.43, 0.47), (7, 6, 5))      # origin, spacing, dims: a grid around the blob, partial bricks


@pytest.fixture(scope="module")
def staged(rt, scenes, blob5k):
    """(the blob scene on the device, the queries as numpy arrays, the same as torch tensors): one upload for the module"""
    import torch
    sp = sd.blob_scene(scenes, blob5k).build_product(rt)
    sp.upload_to_device()
    rng = np.random.default_rng(97)
    # the blob is a bumpy unit sphere: points in a shell around its surface, rays from them in every direction, triangles across it
    u = rng.normal(size=(N, 3))
    pts = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.7, 1.4, (N, 1))).astype(F32)
    tris = (pts[:, None, :] + rng.uniform(-0.15, 0.15, (N, 3, 3))).astype(F32)
    q = dict(o=pts, d=rng.normal(size=(N, 3)).astype(F32), tmax=rng.uniform(0.5, 3.0, N).astype(F32), pts=pts,
             md=rng.uniform(0.1, 0.5, N).astype(F32), tris=tris, skip=rng.integers(-1, 1, N).astype(np.int32))
    edge = rng.uniform(0.05, 0.4, (N, 3))                       # boxes around the same points: some cut the surface, some do not
    q["boxes"] = np.stack([pts - edge / 2, pts + edge / 2], axis=1).astype(F32)
    q["planes"] = np.stack([pts, rng.normal(size=(N, 3))], axis=1).astype(F32)      # planes through the same points: most cut the blob
    # regions (K = 6 boxes) and segments at the same points (drawn last: what is above stays what it was); the triangles above serve
    # closest_to_triangles too
    edge = rng.uniform(0.05, 0.4, (N, 3))
    q["regions"] = rt.regions_from_boxes(np.stack([pts - edge / 2, pts + edge / 2], axis=1).astype(F32))
    q["segs"] = np.stack([pts, pts + rng.uniform(-0.3, 0.3, (N, 3))], axis=1).astype(F32)
    q = {k: np.ascontiguousarray(v) for k, v in q.items()}
    dq = {k: torch.from_numpy(v).cuda() for k, v in q.items()}
    torch.cuda.synchronize()
    yield sp, q, dq
    sp.close()


@pytest.mark.parametrize("name", QUERIES)
def test_stream_object_and_raw_handle_equal_the_numpy_path(staged, name):
    import torch
    sp, q, dq = staged
    assert sorted(_queries(sp, q)) == sorted(QUERIES)
    want = _queries(sp, q)[name]()
    assert all(isinstance(v, np.ndarray) for v in want.values())
    assert any(v.size and np.any(v != v.reshape(-1)[0]) for v in want.values()), "every result is constant: the queries ask nothing"
    s = torch.cuda.Stream()
    current = torch.cuda.current_stream()
    assert s != current
    got = {"stream": _queries(sp, dq, stream=s)[name](), "handle": _queries(sp, dq, stream=s.cuda_stream)[name]()}
    assert torch.cuda.current_stream() == current
    torch.cuda.synchronize()
    for form, res in got.items():
        assert sorted(res) == sorted(want), (form, sorted(res), sorted(want))
        for k, ref in want.items():
            assert res[k].is_cuda, (form, k)
            g = res[k].cpu().numpy()
            assert g.dtype == ref.dtype and g.shape == ref.shape, (form, k, g.dtype, g.shape, ref.dtype, ref.shape)
            assert g.tobytes() == ref.tobytes(), "%s %s: %s differs from the numpy path" % (name, form, k)
