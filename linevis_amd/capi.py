"""ctypes binding of the C-ABI in include/linevis_hip.h (liblinevis_hip.so, HIP / gfx950).

This is plumbing for tests, bench.py and the multi-GPU driver; the product is the shared library.  There is no
CPU fallback: importing works anywhere, but `load()` raises if the library has not been built and every compute
call fails with LV_E_HIP when no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LV_LIB_PATH") or os.path.join(_HERE, "_lib", "liblinevis_hip.so")  # override: kernel tuning builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "linevis_hip.h")

LV_OK = 0
MODE_DEFERRED = 1      # RENDERING_MODE_DEFERRED_SHADING (the tube triangle mesh into a visibility buffer, every pixel shaded once, opaque)
MODE_PPLL = 2          # RENDERING_MODE_PER_PIXEL_LINKED_LIST, src/Renderers/RenderingModes.hpp:32-53
MODE_MLAB = 3          # RENDERING_MODE_MLAB (Multi-Layer Alpha Blending over mode 2's fragments)
MODE_DEPTH_COMPLEXITY = 5   # RENDERING_MODE_DEPTH_COMPLEXITY (fragments per pixel of mode 2's rasterised prism as a colour, and their statistics)
MODE_MBOIT = 6         # RENDERING_MODE_MBOIT (moment-based OIT, power moments as float32, over mode 2's fragments)
MODE_WBOIT = 8         # RENDERING_MODE_WBOIT (weighted blended OIT: five 64-bit sums per pixel over mode 2's fragments)
MODE_DEPTH_PEELING = 9  # RENDERING_MODE_DEPTH_PEELING (every layer of mode 2's fragments in depth order, exactly, no fragment storage)
MODE_ATOMIC_LOOP_64 = 10   # RENDERING_MODE_ATOMIC_LOOP_64 (the K nearest fragments of mode 2 in 64-bit atomicMin slots)
MODE_RAY_TRACER = 11   # RENDERING_MODE_VULKAN_RAY_TRACER

LINE_POINT_DTYPE = np.dtype([("linePosition", "<f4", 3), ("lineAttribute", "<f4"),
                             ("lineTangent", "<f4", 3), ("lineRotation", "<f4"),
                             ("lineNormal", "<f4", 3), ("lineStartIndex", "<u4")])
assert LINE_POINT_DTYPE.itemsize == 48
# struct TubeTriangleVertexData, src/LineData/LineRenderData.hpp:171-176
TUBE_VERTEX_DTYPE = np.dtype([("vertexPosition", "<f4", 3), ("vertexLinePointIndex", "<u4"),
                              ("vertexNormal", "<f4", 3), ("phi", "<f4")])
assert TUBE_VERTEX_DTYPE.itemsize == 32


class Stats(C.Structure):
    _fields_ = [("rays_traced", C.c_uint64), ("nodes_visited", C.c_uint64), ("prims_tested", C.c_uint64),
                ("hits_shaded", C.c_uint64), ("fragments", C.c_uint64), ("ao_hit_pixels", C.c_uint64),
                ("max_depth_complexity", C.c_uint32), ("bvh_depth", C.c_uint32), ("num_segments", C.c_uint32),
                ("num_nodes", C.c_uint32),
                ("ms_accel_build", C.c_float), ("ms_depth_range", C.c_float), ("ms_ao", C.c_float),
                ("ms_color", C.c_float), ("ms_ppll_clear", C.c_float), ("ms_ppll_gather", C.c_float),
                ("ms_ppll_resolve", C.c_float), ("ms_total", C.c_float), ("device_bytes", C.c_uint64),
                ("ms_kernel_avg", C.c_float * 8), ("kernel_launches", C.c_uint32 * 8),
                ("ao_rays_traced", C.c_uint64), ("ao_nodes_visited", C.c_uint64), ("ao_prims_tested", C.c_uint64),
                ("ao_phase_iterations", C.c_uint64 * 3), ("ao_phase_lanes", C.c_uint64 * 3),
                ("max_nodes_per_pixel", C.c_uint32), ("num_tube_triangles", C.c_uint32),
                ("ppll_pool_nodes", C.c_uint64), ("ao_prim_hits", C.c_uint64), ("ao_prim_may_axis", C.c_uint64),
                ("ao_prim_may_both", C.c_uint64),
                ("ms_tri_accel_build", C.c_float), ("ms_tessellate", C.c_float), ("ms_line_points", C.c_float),
                ("num_tri_nodes", C.c_uint32), ("tri_leaf_bytes", C.c_uint32), ("mboit_degenerate_pixels", C.c_uint32)]

    def as_dict(self):
        d = {}
        for n, _ in self._fields_:
            v = getattr(self, n)
            d[n] = list(v) if hasattr(v, "__len__") else v
        return d


class StreamlineSettings(C.Structure):
    """lv_streamline_settings (StreamlineTracingSettings, StreamlineTracingDefines.hpp:144-177)."""
    _fields_ = [("integration_method", C.c_uint32), ("integration_direction", C.c_uint32),
                ("time_step_scale", C.c_float), ("max_num_iterations", C.c_int32),
                ("termination_distance", C.c_float), ("minimum_length", C.c_float)]


class HelicitySeedingSettings(C.Structure):
    """lv_helicity_seeding_settings (the seeder-related members of StreamlineTracingSettings, StreamlineTracingDefines.hpp:156-174)."""
    _fields_ = [("minimum_separation_distance", C.c_float), ("termination_check_type", C.c_uint32), ("loop_check_mode", C.c_uint32),
                ("termination_distance_self", C.c_float), ("seeding_subsampling_factor", C.c_int32)]

    def __init__(self, minimum_separation_distance=0.08, termination_check_type=1, loop_check_mode=1, termination_distance_self=1.0,
                 seeding_subsampling_factor=1):
        super().__init__(minimum_separation_distance, termination_check_type, loop_check_mode, termination_distance_self,
                         seeding_subsampling_factor)


# STREAMLINE_INTEGRATION_METHOD_NAMES / ..._DIRECTION_NAMES, StreamlineTracingDefines.hpp:77-88
INTEGRATION_METHODS = {"Explicit Euler": 0, "Implicit Euler": 1, "Heun": 2, "Midpoint": 3, "Runge-Kutta 4th Order": 4,
                       "Runge-Kutta-Fehlberg": 5}
INTEGRATION_DIRECTIONS = {"Forward": 0, "Backward": 1, "Forward & Backward": 2}


def streamline_settings(method="Runge-Kutta 4th Order", direction="Forward & Backward", time_step_scale=1.0,
                        max_num_iterations=2000, termination_distance=1.0, minimum_length=0.7):
    return StreamlineSettings(INTEGRATION_METHODS[method], INTEGRATION_DIRECTIONS[direction], time_step_scale,
                              max_num_iterations, termination_distance, minimum_length)


KERNEL_AO_PRIMARY, KERNEL_AO_RAYS, KERNEL_RENDER_RT, KERNEL_PPLL_GATHER, KERNEL_PPLL_RESOLVE, KERNEL_DEPTH_RANGE = range(6)
KERNEL_HULL = 8        # LV_KERNEL_HULL: the simulation-mesh hull pass (kernel_times(); lv_stats' arrays keep the eight KERNEL_NAMES)
# the passes of the spatial-hashing denoiser (LV_KERNEL_SH_*): k_sh_write, k_sh_read, the three a-trous passes of its tail together
KERNEL_SH_WRITE, KERNEL_SH_READ, KERNEL_SH_TAIL = 9, 10, 11
KERNEL_NAMES = ["k_ao_primary", "k_ao_rays", "k_render_rt", "k_ppll_gather", "k_ppll_resolve", "k_depth_minmax", "k_ppll_shade_prism",
                "k_ppll_raster_prism"]


class TrajectoryBands(C.Structure):
    """lv_trajectory_bands"""
    _fields_ = [("ribbon_directions", C.c_void_p), ("helicity", C.c_void_p), ("max_helicity", C.c_float)]


class LineVisError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("linevis_hip error %d: %s" % (code, message))
        self.code = code


# every symbol include/linevis_hip.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = ["lv_create", "lv_destroy", "lv_last_error", "lv_version", "lv_set_stream", "lv_set_lines",
           "lv_set_transfer_function", "lv_set_twist_line_texture", "lv_set_camera", "lv_set_background", "lv_set_option", "lv_build_accel",
           "lv_render", "lv_render_device", "lv_render_tiles_device", "lv_get_stats", "lv_reset_timers", "lv_get_kernel_times", "lv_get_ao_tile_costs", "lv_get_dispatch_order", "lv_trace_rays",
           "lv_compute_depth_range", "lv_get_ao", "lv_ppll_get_buffers", "lv_ppll_resolve_buffers", "lv_mlab_resolve_buffers", "lv_mboit_resolve_buffers", "lv_mboit_get_moments", "lv_atomic_loop_get_num_layers", "lv_atomic_loop_get_buffers", "lv_atomic_loop_resolve_buffers", "lv_wboit_get_buffers", "lv_wboit_resolve_buffers",
           "lv_depth_complexity_get_buffers", "lv_depth_complexity_get_stats", "lv_depth_peeling_get_buffers", "lv_depth_peeling_resolve_buffers", "lv_deferred_get_buffers", "lv_deferred_shade_buffers", "lv_svgf_denoise_buffers", "lv_get_accel",
           "lv_spatial_hashing_denoise_buffers", "lv_spatial_hashing_reset", "lv_spatial_hashing_get_cells", "lv_spatial_hashing_get_stats",
           "lv_set_tube_triangle_mesh", "lv_trace_rays_triangles", "lv_set_flow_grid", "lv_trace_streamlines", "lv_trace_streamlines_max_helicity_first",
           "lv_get_streamlines", "lv_get_streamline_seed_indices", "lv_set_ao_parametrization", "lv_get_baked_ao", "lv_bake_ao_start", "lv_bake_ao_poll", "lv_get_mlat_trace", "lv_selftest_rsqrt", "lv_selftest_eval", "lv_selftest_stack",
           "lv_set_trajectories", "lv_set_trajectories_with_bands", "lv_get_lines", "lv_get_tube_triangle_mesh",
           "lv_set_hull_mesh", "lv_get_hull_mesh", "lv_hull_get_fragments", "lv_trace_rays_hull", "lv_rt_get_hits", "lv_line_quads_get_fragments",
           "lv_create_multi", "lv_multi_ranks", "lv_multi_rank_stats", "lv_multi_rebalance", "lv_multi_deal", "lv_tile_deal", "lv_make_tiles"]

# function -> (LV_FN_* id, argument words, result words) of lv_selftest_eval
SELFTEST_FUNCTIONS = {"sincos2pi": (1, 1, 2), "sincos_rad": (2, 1, 2), "atan2_det": (3, 2, 1), "pow_det": (4, 2, 1), "log2_det": (5, 1, 1),
                      "exp2_det": (6, 1, 1), "rsqrt_shade": (7, 1, 1), "tea": (8, 2, 1), "rnd": (9, 1, 2), "transfer_function": (10, 1, 4),
                      "twist_sample": (11, 4, 4), "pack_unorm4x8": (12, 4, 1), "unpack_unorm4x8": (13, 1, 4), "store_rgba8": (14, 4, 1),
                      "mboit_fixed": (15, 1, 2), "mboit_unfixed": (16, 2, 1), "mboit_saturate": (17, 1, 1), "rsqrt_fast": (18, 1, 1),
                      "div_fast": (19, 2, 1), "pow_fast": (20, 2, 1)}

_lib = None


def load():
    """Loads liblinevis_hip.so (built in-tree by linevis_amd/build.py); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: torch ships its own libamdhip64.so (SONAME libamdhip64.so.7).  Importing torch
    # first makes the loader resolve this library's libamdhip64.so.7 dependency to the copy torch already mapped, so
    # device pointers, streams and events are interchangeable with torch tensors / torch.distributed (RCCL).  If the
    # library were loaded first, /opt/rocm's runtime would come in and torch would later map a second one that
    # cannot see the GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, f32, i32, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.c_int, C.c_char_p
    L.lv_create.restype = vp
    L.lv_create.argtypes = [i32, C.POINTER(i32)]
    L.lv_destroy.restype = None
    L.lv_destroy.argtypes = [vp]
    L.lv_last_error.restype = cp
    L.lv_last_error.argtypes = [vp]
    L.lv_version.restype = cp
    L.lv_version.argtypes = []
    L.lv_create_multi.restype = vp
    L.lv_create_multi.argtypes = [vp, i32, cp, C.POINTER(i32)]
    L.lv_multi_ranks.restype = i32
    L.lv_multi_ranks.argtypes = [vp]
    L.lv_make_tiles.restype = u32
    L.lv_make_tiles.argtypes = [u32, u32, u32, u32, u32, vp, u32]
    for name, args in [
        ("lv_multi_rebalance", [vp, C.c_double]),
        ("lv_multi_rank_stats", [vp, i32, vp]),
        ("lv_bake_ao_start", [vp]),
        ("lv_bake_ao_poll", [vp, C.POINTER(i32), C.POINTER(i32)]),
        ("lv_multi_deal", [vp, vp, u32, C.POINTER(u32)]),
        ("lv_tile_deal", [vp, u32, u32, vp]),
        ("lv_set_stream", [vp, vp]),
        ("lv_set_lines", [vp, vp, u32, vp, u32]),
        ("lv_set_transfer_function", [vp, vp, u32, f32, f32]),
        ("lv_set_twist_line_texture", [vp, vp, u32, u32]),
        ("lv_set_camera", [vp, vp, vp, f32, f32, f32, u32, u32]),
        ("lv_set_background", [vp, vp]),
        ("lv_set_option", [vp, cp, cp]),
        ("lv_build_accel", [vp]),
        ("lv_render", [vp, i32, u32, u32, u32, u32, vp]),
        ("lv_render_device", [vp, i32, u32, u32, u32, u32, vp]),
        ("lv_render_tiles_device", [vp, i32, vp, u32, u32, u32, vp]),
        ("lv_get_stats", [vp, C.POINTER(Stats)]),
        ("lv_reset_timers", [vp]),
        ("lv_get_kernel_times", [vp, i32, vp, u32, C.POINTER(u32)]),
        ("lv_get_ao_tile_costs", [vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        ("lv_get_dispatch_order", [vp, vp, vp, u32, C.POINTER(u32)]),
        ("lv_trace_rays", [vp, vp, vp, f32, f32, u32, vp, vp, vp]),
        ("lv_compute_depth_range", [vp, vp]),
        ("lv_get_ao", [vp, vp]),
        ("lv_ppll_get_buffers", [vp, vp, u64, vp, u64, C.POINTER(u32)]),
        ("lv_ppll_resolve_buffers", [vp, vp, u64, vp, u64, u32, u32, u32, u32, vp]),
        ("lv_mlab_resolve_buffers", [vp, vp, u64, vp, u32, u32, vp]),
        ("lv_mboit_resolve_buffers", [vp, vp, u64, vp, u32, u32, C.c_float, C.c_float, vp, vp]),
        ("lv_mboit_get_moments", [vp, vp, u64]),
        ("lv_atomic_loop_get_num_layers", [vp, C.POINTER(u32)]),
        ("lv_atomic_loop_get_buffers", [vp, vp, vp, u64]),
        ("lv_atomic_loop_resolve_buffers", [vp, vp, u64, vp, u32, u32, vp, vp, vp]),
        ("lv_wboit_get_buffers", [vp, vp, vp, u64]),
        ("lv_wboit_resolve_buffers", [vp, vp, u64, vp, u32, u32, vp, vp]),
        ("lv_depth_complexity_get_buffers", [vp, vp, u64]),
        ("lv_depth_complexity_get_stats", [vp, vp]),
        ("lv_depth_peeling_get_buffers", [vp, vp, vp, vp, u64]),
        ("lv_depth_peeling_resolve_buffers", [vp, vp, u64, vp, u32, u32, vp, vp, vp]),
        ("lv_deferred_get_buffers", [vp, vp, vp, u64]),
        ("lv_deferred_shade_buffers", [vp, vp, vp, u32, u32, vp]),
        ("lv_set_hull_mesh", [vp, vp, u32, vp, vp, u32]),
        ("lv_get_hull_mesh", [vp, vp, u32, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        ("lv_hull_get_fragments", [vp, vp, vp, vp, vp, u64, C.POINTER(u64)]),
        ("lv_line_quads_get_fragments", [vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]),
        ("lv_svgf_denoise_buffers", [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]),
        ("lv_spatial_hashing_denoise_buffers", [vp, u32, u32, vp, vp, vp, vp, vp, vp]),
        ("lv_spatial_hashing_reset", [vp, i32]),
        ("lv_spatial_hashing_get_cells", [vp, i32, vp, vp, u64, C.POINTER(u64)]),
        ("lv_spatial_hashing_get_stats", [vp, i32, vp]),
        ("lv_get_accel", [vp, vp, u64, vp, u64]),
        ("lv_set_tube_triangle_mesh", [vp, vp, u32, vp, u32, vp, u32]),
        ("lv_set_trajectories", [vp, vp, vp, vp, u32]),
        ("lv_set_trajectories_with_bands", [vp, vp, vp, vp, u32, C.POINTER(TrajectoryBands)]),
        ("lv_get_lines", [vp, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
        ("lv_get_tube_triangle_mesh", [vp, vp, u32, vp, u32, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        ("lv_trace_rays_triangles", [vp, vp, vp, f32, f32, u32, vp, vp, vp]),
        ("lv_set_flow_grid", [vp, vp, u32, u32, u32, f32, f32, f32, vp, u32]),
        ("lv_trace_streamlines", [vp, vp, u32, C.POINTER(StreamlineSettings), C.POINTER(u64), C.POINTER(u64)]),
        ("lv_trace_streamlines_max_helicity_first", [vp, vp, C.POINTER(StreamlineSettings), C.POINTER(HelicitySeedingSettings),
                                                     C.POINTER(u64), C.POINTER(u64)]),
        ("lv_get_streamlines", [vp, vp, vp, vp]),
        ("lv_get_streamline_seed_indices", [vp, vp]),
        ("lv_set_ao_parametrization", [vp, vp, u32, vp, u32]),
        ("lv_get_baked_ao", [vp, vp, u64]),
        ("lv_get_mlat_trace", [vp, vp, u64, C.POINTER(u64)]),
        ("lv_trace_rays_hull", [vp, vp, vp, f32, f32, u32, vp, vp, vp]),
        ("lv_rt_get_hits", [vp, vp, u64, C.POINTER(u64)]),
        ("lv_selftest_rsqrt", [vp, C.POINTER(u64), C.POINTER(u32)]),
        ("lv_selftest_eval", [vp, u32, vp, u64, vp]),
        ("lv_selftest_stack", [vp, u32, u32, vp, u32, vp, vp, vp]),
    ]:
        fn = getattr(L, name)
        fn.restype = i32
        fn.argtypes = args
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _given_lists(offsets, w, h):
    """What the *_resolve methods share: the offsets of a w x h rectangle as contiguous uint64 (w * h + 1 of them) and the
    (h, w, 4) uint8 image the call fills."""
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    if o.shape[0] != w * h + 1:
        raise ValueError("offsets must hold w * h + 1 values")
    return o, np.empty((h, w, 4), dtype=np.uint8)


def tile_deal(costs, num_tiles, num_ranks):
    """lv_tile_deal: tile -> rank, longest processing time first (costs None: round robin).  Pure host code."""
    out = np.zeros(max(int(num_tiles), 1), dtype=np.uint32)
    c = np.ascontiguousarray(costs, dtype=np.float64) if costs is not None else None
    rc = load().lv_tile_deal(_p(c) if c is not None else None, int(num_tiles), int(num_ranks), _p(out))
    if rc != LV_OK:
        raise LineVisError(rc, "lv_tile_deal")
    return out[:int(num_tiles)]


def make_tiles(x0, y0, w, h, tile):
    """lv_make_tiles: origins of the tile x tile squares covering the rectangle, along a Morton order.  Pure host code."""
    L = load()
    n = L.lv_make_tiles(int(x0), int(y0), int(w), int(h), int(tile), None, 0)
    out = np.zeros((max(n, 1), 2), dtype=np.uint32)
    L.lv_make_tiles(int(x0), int(y0), int(w), int(h), int(tile), _p(out), n)
    return out[:n]


def _fmt(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (float, np.floating)):
        return "%.9g" % float(v)  # round-trips float32
    return str(v)


class Context:
    """One renderer context on one HIP device (thin OO veneer over the lv_* calls)."""

    def __init__(self, device=0, devices=None, transport="rccl"):
        """device: one HIP device.  devices = [d0, d1, ...]: lv_create_multi -- one context per device behind this handle, frames
        sharded by screen tiles and gathered on d0 (transport "rccl" | "memcpy")."""
        self.L = load()
        err = C.c_int(0)
        if devices is not None:
            devs = np.ascontiguousarray(devices, dtype=np.int32)
            self.h = self.L.lv_create_multi(_p(devs), len(devs), transport.encode("utf-8"), C.byref(err))
            if not self.h:
                raise LineVisError(err.value, "lv_create_multi(%s, %s) failed" % (list(devs), transport))
            device = int(devs[0])
        else:
            self.h = self.L.lv_create(int(device), C.byref(err))
            if not self.h:
                raise LineVisError(err.value, "lv_create(%d) failed: no usable HIP device (no CPU fallback)" % device)
        self.width = self.height = 0
        self.device = int(device)

    @property
    def num_ranks(self):
        return int(self.L.lv_multi_ranks(self.h))

    def rebalance(self, base_cost_per_tile=4.0 * 64 * 64):
        """Multi-device handle: re-deal the tiles of the last frame by measured cost (lv_multi_rebalance)."""
        self._ck(self.L.lv_multi_rebalance(self.h, float(base_cost_per_tile)))

    def deal(self):
        """tile -> rank of the last frame of a multi-device handle"""
        n = C.c_uint32(0)
        self._ck(self.L.lv_multi_deal(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._ck(self.L.lv_multi_deal(self.h, _p(out), len(out), C.byref(n)))
        return out[:n.value]

    def close(self):
        if getattr(self, "h", None):
            self.L.lv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != LV_OK:
            raise LineVisError(rc, self.L.lv_last_error(self.h).decode("utf-8", "replace"))

    def set_stream(self, stream_handle):
        self._ck(self.L.lv_set_stream(self.h, C.c_void_p(stream_handle) if stream_handle else None))

    def set_lines(self, points, seg_indices):
        pts = np.ascontiguousarray(points, dtype=LINE_POINT_DTYPE)
        seg = np.ascontiguousarray(seg_indices, dtype=np.uint32).reshape(-1, 2)
        self._ck(self.L.lv_set_lines(self.h, _p(pts), len(pts), _p(seg), len(seg)))

    def set_tube_triangle_mesh(self, triangle_indices, vertices, line_points):
        idx = np.ascontiguousarray(triangle_indices, dtype=np.uint32).reshape(-1, 3)
        v = np.ascontiguousarray(vertices, dtype=TUBE_VERTEX_DTYPE)
        pts = np.ascontiguousarray(line_points, dtype=LINE_POINT_DTYPE)
        self._ck(self.L.lv_set_tube_triangle_mesh(self.h, _p(idx), len(idx), _p(v), len(v), _p(pts), len(pts)))

    def set_trajectories(self, positions, attribute, line_offsets, ribbon_directions=None, helicity=None, max_helicity=0.0):
        """lv_set_trajectories: the trajectories go to HBM, line points / index pairs / tube mesh are written by kernels.
        ribbon_directions (one vec3 per point: band data) and / or helicity (one float per point; max_helicity <= 0: max |helicity|,
        reduced on the device) go along through lv_set_trajectories_with_bands."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        off = np.ascontiguousarray(line_offsets, dtype=np.uint32)
        att = None if attribute is None else np.ascontiguousarray(attribute, dtype=np.float32).reshape(-1)
        if len(off) < 1 or int(off[-1]) != len(pos) or (att is not None and len(att) != len(pos)):
            raise ValueError("line_offsets[-1] must equal the number of points (and of attribute values)")
        if ribbon_directions is None and helicity is None:
            self._ck(self.L.lv_set_trajectories(self.h, _p(pos), None if att is None else _p(att), _p(off), len(off) - 1))
            return
        rib = None if ribbon_directions is None else np.ascontiguousarray(ribbon_directions, dtype=np.float32)
        hel = None if helicity is None else np.ascontiguousarray(helicity, dtype=np.float32)
        if rib is not None and (rib.size != 3 * len(pos) or (rib.ndim == 2 and rib.shape[1] != 3)):
            raise ValueError("ribbon_directions must hold one vec3 per point (%d points, got shape %s)" % (len(pos), rib.shape))
        if hel is not None and hel.size != len(pos):
            raise ValueError("helicity must hold one float per point (%d points, got %d)" % (len(pos), hel.size))
        bands = TrajectoryBands(None if rib is None else _p(rib), None if hel is None else _p(hel), float(max_helicity))
        self._ck(self.L.lv_set_trajectories_with_bands(self.h, _p(pos), None if att is None else _p(att), _p(off), len(off) - 1,
                                                       C.byref(bands)))

    def get_lines(self):
        """(points, segment index pairs) as they sit in HBM (lv_set_lines' input or lv_set_trajectories' device output)."""
        n, m = C.c_uint32(), C.c_uint32()
        self._ck(self.L.lv_get_lines(self.h, None, 0, None, 0, C.byref(n), C.byref(m)))
        pts = np.zeros(n.value, dtype=LINE_POINT_DTYPE)
        seg = np.zeros((m.value, 2), dtype=np.uint32)
        self._ck(self.L.lv_get_lines(self.h, _p(pts), n.value, _p(seg), m.value, None, None))
        return pts, seg

    def get_tube_triangle_mesh(self):
        """(triangle indices [n, 3], vertices, line points) of the current tube mesh (tessellated on the device if need be)."""
        nt, nv, npnt = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.lv_get_tube_triangle_mesh(self.h, None, 0, None, 0, None, 0, C.byref(nt), C.byref(nv), C.byref(npnt)))
        idx = np.zeros((nt.value, 3), dtype=np.uint32)
        v = np.zeros(nv.value, dtype=TUBE_VERTEX_DTYPE)
        pts = np.zeros(npnt.value, dtype=LINE_POINT_DTYPE)
        self._ck(self.L.lv_get_tube_triangle_mesh(self.h, _p(idx), nt.value, _p(v), nv.value, _p(pts), npnt.value, None, None, None))
        return idx, v, pts

    def set_hull_mesh(self, triangle_indices, positions, normals):
        """lv_set_hull_mesh: the simulation-mesh hull, triangle indices [n, 3], positions and normals [m, 3] (normals are used as given).
        No triangles (None or empty) removes the mesh.  Drawn by modes 5, 8 and 10 once hull_opacity has been set to a value > 0 (mode 11 under hull_ray_tracing = on, modes 2 and 3 under
        hull_fragment_pool = on)."""
        idx = np.ascontiguousarray(triangle_indices if triangle_indices is not None else [], dtype=np.uint32).reshape(-1, 3)
        if len(idx) == 0:
            self._ck(self.L.lv_set_hull_mesh(self.h, None, 0, None, None, 0))
            return
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if len(nrm) != len(pos):
            raise ValueError("one normal per position")
        self._ck(self.L.lv_set_hull_mesh(self.h, _p(idx), len(idx), _p(pos), _p(nrm), len(pos)))

    def get_hull_mesh(self):
        """(triangle indices [n, 3], positions [m, 3], normals [m, 3]) of the current hull mesh (lv_get_hull_mesh)"""
        nt, nv = C.c_uint32(), C.c_uint32()
        self._ck(self.L.lv_get_hull_mesh(self.h, None, 0, None, None, 0, C.byref(nt), C.byref(nv)))
        idx = np.zeros((nt.value, 3), dtype=np.uint32)
        pos = np.zeros((nv.value, 3), dtype=np.float32)
        nrm = np.zeros((nv.value, 3), dtype=np.float32)
        self._ck(self.L.lv_get_hull_mesh(self.h, _p(idx), nt.value, _p(pos), _p(nrm), nv.value, None, None))
        return idx, pos, nrm

    def hull_fragments(self, capacity=None):
        """lv_hull_get_fragments: every kept hull fragment of the viewport under the current camera and options, unordered:
        (pixel = y * width + x, triangle, window depth, straight rgba [n, 4]).  capacity None: as many as there are."""
        n = C.c_uint64(0)
        if capacity is None:
            rc = self.L.lv_hull_get_fragments(self.h, None, None, None, None, 0, C.byref(n))
            if rc not in (LV_OK, -4):
                self._ck(rc)
            capacity = n.value
        cap = max(int(capacity), 1)
        pix, tri = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        z, rgba = np.zeros(cap, dtype=np.float32), np.zeros((cap, 4), dtype=np.float32)
        self._ck(self.L.lv_hull_get_fragments(self.h, _p(pix), _p(tri), _p(z), _p(rgba), int(capacity), C.byref(n)))
        k = n.value
        return pix[:k], tri[:k], z[:k], rgba[:k]

    def line_quad_fragments(self, capacity=None):
        """lv_line_quads_get_fragments: every kept line-quad fragment of the last whole-viewport mode-5, 8 or 10 frame drawn with line_primitive_mode =
        "Quads (Programmable Pull)", unordered: (pixel = y * width + x, segment, triangle 0 | 1, window depth, straight rgba [n, 4]).
        capacity None: as many as there are."""
        n = C.c_uint64(0)
        if capacity is None:
            rc = self.L.lv_line_quads_get_fragments(self.h, 0, None, None, None, None, None, C.byref(n))
            if rc not in (LV_OK, -4):
                self._ck(rc)
            capacity = n.value
        cap = max(int(capacity), 1)
        pix, seg, tri = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        z, rgba = np.zeros(cap, dtype=np.float32), np.zeros((cap, 4), dtype=np.float32)
        self._ck(self.L.lv_line_quads_get_fragments(self.h, int(capacity), _p(pix), _p(seg), _p(tri), _p(z), _p(rgba), C.byref(n)))
        k = n.value
        return pix[:k], seg[:k], tri[:k], z[:k], rgba[:k]

    def set_transfer_function(self, rgba, attr_min=0.0, attr_max=1.0):
        tf = np.ascontiguousarray(rgba, dtype=np.float32).reshape(-1, 4)
        self._ck(self.L.lv_set_transfer_function(self.h, _p(tf), tf.shape[0], attr_min, attr_max))

    def set_twist_line_texture(self, rgba8):
        """Twist-line texture of the rotating helicity bands: (h, w, 4) uint8, or None to unload."""
        if rgba8 is None:
            self._ck(self.L.lv_set_twist_line_texture(self.h, None, 0, 0))
            return
        img = np.ascontiguousarray(rgba8, dtype=np.uint8)
        self._ck(self.L.lv_set_twist_line_texture(self.h, _p(img), img.shape[1], img.shape[0]))

    def set_camera(self, view, proj, fov_y, near, far, width, height):
        v = np.ascontiguousarray(view, dtype=np.float32).reshape(16)
        p = np.ascontiguousarray(proj, dtype=np.float32).reshape(16)
        self._ck(self.L.lv_set_camera(self.h, _p(v), _p(p), fov_y, near, far, int(width), int(height)))
        self.width, self.height = int(width), int(height)

    def set_background(self, rgba):
        b = np.ascontiguousarray(rgba, dtype=np.float32).reshape(4)
        self._ck(self.L.lv_set_background(self.h, _p(b)))

    def set_option(self, key, value):
        self._ck(self.L.lv_set_option(self.h, key.encode(), _fmt(value).encode()))
        if key == "mboit_num_moments":
            self._mboit_num_moments = int(value)
        if key == "atomic_loop_num_layers":
            self._atomic_loop_num_layers = int(value)

    def set_options(self, settings):
        """LineRenderer::setNewSettings(const SettingsMap&): a dict of string keys."""
        for k, v in settings.items():
            self.set_option(k, v)

    def build_accel(self):
        self._ck(self.L.lv_build_accel(self.h))

    def render(self, mode=MODE_RAY_TRACER, tile=None, out=None):
        x0, y0, w, h = tile if tile is not None else (0, 0, self.width, self.height)
        if out is None:
            out = np.empty((h, w, 4), dtype=np.uint8)
        assert out.shape == (h, w, 4) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        self._ck(self.L.lv_render(self.h, mode, x0, y0, w, h, _p(out)))
        return out

    def render_device(self, out_ptr, mode=MODE_RAY_TRACER, tile=None):
        x0, y0, w, h = tile if tile is not None else (0, 0, self.width, self.height)
        self._ck(self.L.lv_render_device(self.h, mode, x0, y0, w, h, C.c_void_p(out_ptr)))

    def render_tiles_device(self, out_ptr, tiles_xy, tile_w, tile_h, mode=MODE_RAY_TRACER):
        t = np.ascontiguousarray(tiles_xy, dtype=np.uint32).reshape(-1, 2)
        self._ck(self.L.lv_render_tiles_device(self.h, mode, _p(t), t.shape[0], tile_w, tile_h, C.c_void_p(out_ptr)))

    def stats(self):
        s = Stats()
        self._ck(self.L.lv_get_stats(self.h, C.byref(s)))
        return s

    def reset_timers(self):
        self._ck(self.L.lv_reset_timers(self.h))

    def trace_rays(self, origins, dirs, t_min, t_max):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.empty(n, dtype=np.float32)
        seg = np.empty(n, dtype=np.uint32)
        kind = np.empty(n, dtype=np.uint32)
        self._ck(self.L.lv_trace_rays(self.h, _p(o), _p(d), t_min, t_max, n, _p(t), _p(seg), _p(kind)))
        return t, seg, kind

    def trace_rays_triangles(self, origins, dirs, t_min, t_max):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.empty(n, dtype=np.float32)
        tri = np.empty(n, dtype=np.uint32)
        uv = np.empty((n, 2), dtype=np.float32)
        self._ck(self.L.lv_trace_rays_triangles(self.h, _p(o), _p(d), t_min, t_max, n, _p(t), _p(tri), _p(uv)))
        return t, tri, uv

    def trace_rays_hull(self, origins, dirs, t_min, t_max):
        """lv_trace_rays_hull: the closest hit of every ray with the simulation-mesh hull -> (t, triangle or 0xFFFFFFFF, uv [n, 2])"""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.empty(n, dtype=np.float32)
        tri = np.empty(n, dtype=np.uint32)
        uv = np.empty((n, 2), dtype=np.float32)
        self._ck(self.L.lv_trace_rays_hull(self.h, _p(o), _p(d), t_min, t_max, n, _p(t), _p(tri), _p(uv)))
        return t, tri, uv

    def rt_hits(self):
        """lv_rt_get_hits: the steps of every pixel's loop in the last whole-viewport mode-11 frame rendered with rt_record_hits, as
        (n, 9) uint32 records {pixel, sampleIdx << 16 | hitIdx, bit 31 | hull triangle or segment << 2 | kind, bits of t, of
        payload.hitT and of the straight colour r, g, b, a}, in no particular order."""
        cnt = C.c_uint64()
        self._ck(self.L.lv_rt_get_hits(self.h, None, 0, C.byref(cnt)))
        rec = np.zeros((max(int(cnt.value), 1), 9), dtype=np.uint32)
        self._ck(self.L.lv_rt_get_hits(self.h, _p(rec), rec.shape[0], C.byref(cnt)))
        return rec[:int(cnt.value)]

    def set_ao_parametrization(self, blending_weights, sampling_locations):
        bw = np.ascontiguousarray(blending_weights, dtype=np.float32)
        sl = np.ascontiguousarray(sampling_locations, dtype=np.float32)
        self._ck(self.L.lv_set_ao_parametrization(self.h, _p(bw), len(bw), _p(sl), len(sl)))
        self._bake_shape = len(sl)

    def get_baked_ao(self, num_tube_subdivisions=8):
        out = np.zeros((self._bake_shape, num_tube_subdivisions), dtype=np.float32)
        self._ck(self.L.lv_get_baked_ao(self.h, _p(out), out.size))
        return out

    def set_flow_grid(self, vector_field, spacing, scalar_fields=()):
        """vector_field [zs, ys, xs, 3] float32, scalar_fields: list of [zs, ys, xs] (sampled as line attributes)."""
        v = np.ascontiguousarray(vector_field, dtype=np.float32)
        zs, ys, xs = v.shape[:3]
        sf = [np.ascontiguousarray(f, dtype=np.float32) for f in scalar_fields]
        ptrs = (C.c_void_p * max(len(sf), 1))(*[f.ctypes.data for f in sf])
        self._ck(self.L.lv_set_flow_grid(self.h, _p(v), xs, ys, zs, spacing[0], spacing[1], spacing[2], ptrs, len(sf)))
        self._flow_scalars = len(sf)

    def trace_streamlines(self, seeds, settings):
        """-> (positions [P,3], attributes [k,P], line_offsets [L+1])"""
        sd = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1, 3)
        nl, npt = C.c_uint64(), C.c_uint64()
        self._ck(self.L.lv_trace_streamlines(self.h, _p(sd), len(sd), C.byref(settings), C.byref(nl), C.byref(npt)))
        pos = np.zeros((npt.value, 3), dtype=np.float32)
        att = np.zeros((self._flow_scalars, npt.value), dtype=np.float32)
        off = np.zeros(nl.value + 1, dtype=np.uint32)
        self._ck(self.L.lv_get_streamlines(self.h, _p(pos), _p(att), _p(off)))
        return pos, att, off

    def trace_streamlines_max_helicity_first(self, helicity_field, settings, seeding=None):
        """StreamlineMaxHelicityFirstSeeder: helicity_field [zs, ys, xs] -> (positions [P,3], attributes [k,P], line_offsets [L+1])"""
        hf = np.ascontiguousarray(helicity_field, dtype=np.float32)
        seeding = seeding or HelicitySeedingSettings()
        nl, npt = C.c_uint64(), C.c_uint64()
        self._ck(self.L.lv_trace_streamlines_max_helicity_first(self.h, _p(hf), C.byref(settings), C.byref(seeding), C.byref(nl),
                                                                C.byref(npt)))
        pos = np.zeros((npt.value, 3), dtype=np.float32)
        att = np.zeros((self._flow_scalars, npt.value), dtype=np.float32)
        off = np.zeros(nl.value + 1, dtype=np.uint32)
        self._ck(self.L.lv_get_streamlines(self.h, _p(pos), _p(att), _p(off)))
        return pos, att, off

    def streamline_seed_indices(self, num_lines):
        out = np.zeros(num_lines, dtype=np.uint32)
        self._ck(self.L.lv_get_streamline_seed_indices(self.h, _p(out)))
        return out

    def depth_range(self):
        out = np.empty(2, dtype=np.float32)
        self._ck(self.L.lv_compute_depth_range(self.h, _p(out)))
        return out

    def get_ao(self):
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._ck(self.L.lv_get_ao(self.h, _p(out)))
        return out

    def mlat_trace(self):
        """Candidate visiting order of the last MLAT frame (collect_stats + mlat_record_trace): (n, 4) uint32 records
        {pixel index y * W + x, sequence number, segment, flag 0 = inserted / 1 = dropped (interval already shorter)}."""
        cnt = C.c_uint64()
        self._ck(self.L.lv_get_mlat_trace(self.h, None, 0, C.byref(cnt)))
        rec = np.zeros((max(int(cnt.value), 1), 4), dtype=np.uint32)
        self._ck(self.L.lv_get_mlat_trace(self.h, _p(rec), rec.shape[0], C.byref(cnt)))
        return rec[:int(cnt.value)]

    def selftest_rsqrt(self):
        """(mismatches, bits of one mismatching argument) of the shading code's 1 / sqrt(x) sequence against IEEE division and square
        root over all 2^32 float arguments, evaluated on the device."""
        bad, first = C.c_uint64(), C.c_uint32()
        self._ck(self.L.lv_selftest_rsqrt(self.h, C.byref(bad), C.byref(first)))
        return int(bad.value), int(first.value)

    def selftest_eval(self, name, words):
        """lv_selftest_eval: one build-owned scalar function (SELFTEST_FUNCTIONS) on (n, arity) uint32 bit patterns, evaluated on the
        device by the inline functions the render kernels call -> (n, results) uint32."""
        fid, arity, results = SELFTEST_FUNCTIONS[name]
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, arity)
        out = np.empty((len(w), results), dtype=np.uint32)
        self._ck(self.L.lv_selftest_eval(self.h, fid, _p(w), len(w), _p(out)))
        return out

    def selftest_stack(self, instantiation, wide_levels, ops=None):
        """lv_selftest_stack: the ray kernels' traversal stack on scripts.  instantiation 0 = the RTAO sample kernel's window, 1 = the
        tile kernels'; ops = (256, n, 4) uint32 {code | keep flags << 8, c3, c2, c1} with code 1 = push3, 2 = pop, 3 = clear, 0 = nothing.
        -> (popped words per thread as a list of uint32 arrays, (256, 3) {pops, spills, refills}, info dict); ops = None: info only."""
        info = np.zeros(6, dtype=np.uint64)
        if ops is None:
            self._ck(self.L.lv_selftest_stack(self.h, int(instantiation), int(wide_levels), None, 0, None, None, _p(info)))
            words, counts = [], np.zeros((256, 3), dtype=np.uint32)
        else:
            ops = np.ascontiguousarray(ops, dtype=np.uint32)
            assert ops.ndim == 3 and ops.shape[0] == 256 and ops.shape[2] == 4
            out = np.zeros((256, ops.shape[1]), dtype=np.uint32)
            counts = np.zeros((256, 3), dtype=np.uint32)
            self._ck(self.L.lv_selftest_stack(self.h, int(instantiation), int(wide_levels), _p(ops), ops.shape[1], _p(out), _p(counts), _p(info)))
            words = [out[t, :counts[t, 0]] for t in range(256)]
        keys = ("window", "block", "column_entries", "context_slab_bytes", "wide_levels", "triangle_wide_levels")
        return words, counts, dict(zip(keys, (int(v) for v in info)))

    def kernel_times(self, kernel_id):
        """Individual launch durations (ms) of one kernel since reset_timers(), oldest first (at most the last 512)."""
        out = np.zeros(512, dtype=np.float32)
        cnt = C.c_uint32()
        self._ck(self.L.lv_get_kernel_times(self.h, int(kernel_id), _p(out), 512, C.byref(cnt)))
        return out[:cnt.value].copy()

    def ao_tile_costs(self):
        """Hit pixels of the last RTAO pass per tile of the last tile list (64x64-pixel groups summed per tile)."""
        n, g = C.c_uint32(), C.c_uint32()
        self._ck(self.L.lv_get_ao_tile_costs(self.h, None, 0, C.byref(n), C.byref(g)))
        out = np.zeros(n.value, dtype=np.uint32)
        self._ck(self.L.lv_get_ao_tile_costs(self.h, _p(out), n.value, C.byref(n), C.byref(g)))
        return out.reshape(-1, max(g.value, 1)).sum(axis=1)

    def dispatch_order(self):
        """(order, cost) of the last frame's 64x64-pixel groups: order[k] = group started k-th, cost[g] = ticks group g took."""
        n = C.c_uint32(0)
        self._ck(self.L.lv_get_dispatch_order(self.h, None, None, 0, C.byref(n)))
        order = np.zeros(n.value, dtype=np.uint32)
        cost = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self._ck(self.L.lv_get_dispatch_order(self.h, _p(order), _p(cost), n.value, C.byref(n)))
        return order, cost

    def bake_ao_start(self):
        """queue the static RTAO bake on the context's second stream and return"""
        self._ck(self.L.lv_bake_ao_start(self.h))

    def bake_ao_poll(self):
        """(running, ready) of the asynchronous bake; never blocks"""
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self.L.lv_bake_ao_poll(self.h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def rank_stats(self, rank):
        """lv_stats of one rank of a multi-device handle (nothing summed)."""
        s = Stats()
        self._ck(self.L.lv_multi_rank_stats(self.h, int(rank), C.byref(s)))
        return s

    def ppll_buffers(self, padded_pixels, max_nodes):
        # the library's physical pool may exceed the logical linkedListSize (chunk tails / sub-pools of the gather): room for it
        max_nodes = max(int(max_nodes), int(self.stats().ppll_pool_nodes))
        nodes = np.zeros((max_nodes, 3), dtype=np.uint32)
        start = np.zeros(padded_pixels, dtype=np.uint32)
        cnt = C.c_uint32()
        self._ck(self.L.lv_ppll_get_buffers(self.h, _p(nodes), max_nodes, _p(start), padded_pixels, C.byref(cnt)))
        return nodes, start, cnt.value

    def ppll_resolve(self, nodes, start_offset, tile=None):
        x0, y0, w, h = tile if tile is not None else (0, 0, self.width, self.height)
        n = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 3)
        s = np.ascontiguousarray(start_offset, dtype=np.uint32)
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._ck(self.L.lv_ppll_resolve_buffers(self.h, _p(n), n.shape[0], _p(s), s.shape[0], x0, y0, w, h, _p(out)))
        return out

    def mlab_resolve(self, entries, offsets, w, h):
        """Mode 3's fold of caller-supplied runs (lv_mlab_resolve_buffers): entries = (n, 3) uint32 {colour, depth bits, key},
        pixel p = y * w + x owns entries[offsets[p]:offsets[p + 1]] in any order.  Returns (h, w, 4) uint8."""
        e = np.ascontiguousarray(entries, dtype=np.uint32).reshape(-1, 3)
        o, out = _given_lists(offsets, w, h)
        self._ck(self.L.lv_mlab_resolve_buffers(self.h, _p(e), e.shape[0], _p(o), w, h, _p(out)))
        return out

    def mboit_resolve(self, entries, offsets, w, h, log_depth_min, log_depth_max, num_moments=4):
        """Mode 6's two sweeps over caller-supplied runs (lv_mboit_resolve_buffers) with mboit_num_moments = num_moments: entries =
        (n, 5) float32 {r, g, b, a, view depth}, pixel p = y * w + x owns entries[offsets[p]:offsets[p + 1]] in any order.
        Returns ((h, w, 4) uint8, (h, w, 1 + num_moments) float32: b_0 and the normalised moments)."""
        self.set_option("mboit_num_moments", int(num_moments))
        e = np.ascontiguousarray(entries, dtype=np.float32).reshape(-1, 5)
        o, out = _given_lists(offsets, w, h)
        mom = np.zeros((h, w, 1 + int(num_moments)), dtype=np.float32)
        self._ck(self.L.lv_mboit_resolve_buffers(self.h, _p(e), e.shape[0], _p(o), w, h, float(log_depth_min), float(log_depth_max),
                                                 _p(mom), _p(out)))
        return out, mom

    def mboit_moments(self):
        """The moments of the last mode-6 frame rendered with mboit_fragment_storage = streamed over the whole viewport
        (lv_mboit_get_moments): (height, width, 1 + mboit_num_moments) float32, b_0 then the normalised b_1 ... b_N, zeros where b_0
        is under the threshold."""
        n = getattr(self, "_mboit_num_moments", 4)
        mom = np.zeros((self.height, self.width, 1 + n), dtype=np.float32)
        self._ck(self.L.lv_mboit_get_moments(self.h, _p(mom), mom.size))
        return mom

    def atomic_loop_buffers(self):
        """The slots and tail sums of the last mode-10 frame over the whole viewport (lv_atomic_loop_get_buffers): ((height, width, K)
        uint64 keys, ascending then 0xFFFFFFFFFFFFFFFF; (height, width, 5) uint64 {SA, SR, SG, SB, SL}), K = that frame's
        atomic_loop_num_layers (lv_atomic_loop_get_num_layers), whatever the option has been set to since."""
        k = C.c_uint32(0)
        self._ck(self.L.lv_atomic_loop_get_num_layers(self.h, C.byref(k)))
        k = int(k.value)
        slots = np.zeros((self.height, self.width, k), dtype=np.uint64)
        tail = np.zeros((self.height, self.width, 5), dtype=np.uint64)
        self._ck(self.L.lv_atomic_loop_get_buffers(self.h, _p(slots), _p(tail), self.width * self.height))
        return slots, tail

    def atomic_loop_resolve(self, keys, offsets, w, h):
        """Mode 10's insert and resolve of caller-supplied keys (lv_atomic_loop_resolve_buffers) with K = atomic_loop_num_layers:
        keys = uint64 (depth bits << 32 | packed colour), pixel p = y * w + x owns keys[offsets[p]:offsets[p + 1]].  Returns ((h, w,
        4) uint8, (h, w, K) uint64 slots, (h, w, 5) uint64 tail sums)."""
        k = getattr(self, "_atomic_loop_num_layers", 8)
        e = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        o, out = _given_lists(offsets, w, h)
        slots = np.zeros((h, w, k), dtype=np.uint64)
        tail = np.zeros((h, w, 5), dtype=np.uint64)
        self._ck(self.L.lv_atomic_loop_resolve_buffers(self.h, _p(e), e.shape[0], _p(o), w, h, _p(out), _p(slots), _p(tail)))
        return out, slots, tail

    def wboit_buffers(self):
        """The sums and counts of the last mode-8 frame over the whole viewport (lv_wboit_get_buffers): ((height, width, 5) int64
        {SR, SG, SB, SA, SL} in the 2^-36 fixed point, (height, width) uint32 kept-fragment counts)."""
        sums = np.zeros((self.height, self.width, 5), dtype=np.int64)
        counts = np.zeros((self.height, self.width), dtype=np.uint32)
        self._ck(self.L.lv_wboit_get_buffers(self.h, _p(sums), _p(counts), self.width * self.height))
        return sums, counts

    def wboit_resolve(self, entries, offsets, w, h):
        """Mode 8's accumulation and resolve of caller-supplied fragments (lv_wboit_resolve_buffers) under wboit_depth_weight:
        entries = (n, 5) float32 {r, g, b, alpha, window depth}, pixel p = y * w + x owns entries[offsets[p]:offsets[p + 1]].
        Returns ((h, w, 4) uint8, (h, w, 5) int64 sums)."""
        e = np.ascontiguousarray(entries, dtype=np.float32).reshape(-1, 5)
        o, out = _given_lists(offsets, w, h)
        sums = np.zeros((h, w, 5), dtype=np.int64)
        self._ck(self.L.lv_wboit_resolve_buffers(self.h, _p(e), e.shape[0], _p(o), w, h, _p(out), _p(sums)))
        return out, sums

    def depth_complexity_buffers(self):
        """The kept-fragment counts of the last mode-5 frame over the whole viewport (lv_depth_complexity_get_buffers): (height,
        width) uint32."""
        counts = np.zeros((self.height, self.width), dtype=np.uint32)
        self._ck(self.L.lv_depth_complexity_get_buffers(self.h, _p(counts), self.width * self.height))
        return counts

    def depth_complexity_stats(self):
        """The device-side reduction of the last mode-5 frame's counts (lv_depth_complexity_get_stats): a dict with total,
        used_locations, max, min and buffer_size."""
        v = np.zeros(5, dtype=np.uint64)
        self._ck(self.L.lv_depth_complexity_get_stats(self.h, _p(v)))
        return dict(zip(("total", "used_locations", "max", "min", "buffer_size"), (int(x) for x in v)))

    def depth_peeling_buffers(self):
        """The accumulators, layer counts and kept-fragment counts of the last mode-9 frame over the whole viewport
        (lv_depth_peeling_get_buffers): ((height, width, 4) float32 premultiplied, (height, width) uint32, (height, width) uint32)."""
        accum = np.zeros((self.height, self.width, 4), dtype=np.float32)
        layers = np.zeros((self.height, self.width), dtype=np.uint32)
        counts = np.zeros((self.height, self.width), dtype=np.uint32)
        self._ck(self.L.lv_depth_peeling_get_buffers(self.h, _p(accum), _p(layers), _p(counts), self.width * self.height))
        return accum, layers, counts

    def depth_peeling_resolve(self, rgba, z, keys, offsets, w, h):
        """Mode 9's passes and blit on caller-supplied fragments (lv_depth_peeling_resolve_buffers) under depth_peeling_max_layers:
        rgba = (n, 4) float32 straight colours, z = (n,) float32 window depths, keys = (n,) uint32 primitive keys (distinct within a
        pixel), pixel p = y * w + x owns entries offsets[p]:offsets[p + 1].  Returns ((h, w, 4) uint8, (h, w, 4) float32 accumulators,
        (h, w) uint32 layer counts)."""
        c = np.ascontiguousarray(rgba, dtype=np.float32).reshape(-1, 4)
        e = np.empty((c.shape[0], 6), dtype=np.uint32)
        e[:, :4] = c.view(np.uint32)
        e[:, 4] = np.ascontiguousarray(z, dtype=np.float32).reshape(-1).view(np.uint32)
        e[:, 5] = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
        o, out = _given_lists(offsets, w, h)
        accum = np.zeros((h, w, 4), dtype=np.float32)
        layers = np.zeros((h, w), dtype=np.uint32)
        self._ck(self.L.lv_depth_peeling_resolve_buffers(self.h, _p(e), e.shape[0], _p(o), w, h, _p(out), _p(accum), _p(layers)))
        return out, accum, layers

    def deferred_buffers(self):
        """The visibility buffer of the last mode-1 frame over the whole viewport (lv_deferred_get_buffers): ((height, width) uint32
        primitive indices, 0xFFFFFFFF = none; (height, width) float32 depths, 1.0 = none)."""
        prim = np.zeros((self.height, self.width), dtype=np.uint32)
        depth = np.zeros((self.height, self.width), dtype=np.float32)
        self._ck(self.L.lv_deferred_get_buffers(self.h, _p(prim), _p(depth), self.width * self.height))
        return prim, depth

    def deferred_shade(self, primitive_index, depth):
        """Mode 1's shading pass on a caller-supplied visibility buffer (lv_deferred_shade_buffers): primitive_index (h, w) uint32,
        depth (h, w) float32; (w, h) is the viewport size of the shading.  Returns (h, w, 4) uint8."""
        prim = np.ascontiguousarray(primitive_index, dtype=np.uint32)
        z = np.ascontiguousarray(depth, dtype=np.float32)
        if prim.ndim != 2 or z.shape != prim.shape:
            raise ValueError("primitive_index and depth must be (h, w)")
        h, w = prim.shape
        out = np.zeros((h, w, 4), dtype=np.uint8)
        self._ck(self.L.lv_deferred_shade_buffers(self.h, _p(prim), _p(z), w, h, _p(out)))
        return out

    def svgf_denoise(self, noisy, normal_depth, flow_fwidth, color_history, moments_history, normal_depth_history):
        """One SVGF denoise() on caller-supplied images (lv_svgf_denoise_buffers): noisy (h, w), normal_depth (h, w, 4), flow_fwidth
        (h, w, 4) {flow x, flow y, depth fwidth, unused}; the history images color_history (h, w), moments_history (h, w, 4) and
        normal_depth_history (h, w, 4) must be C-contiguous float32 arrays and are updated in place.  Returns the denoised (h, w)
        image.  Iterations and thresholds are the context's svgf_denoiser_* options."""
        a = np.ascontiguousarray(noisy, dtype=np.float32)
        h, w = a.shape
        nd = np.ascontiguousarray(normal_depth, dtype=np.float32)
        ff = np.ascontiguousarray(flow_fwidth, dtype=np.float32)
        if nd.shape != (h, w, 4) or ff.shape != (h, w, 4):
            raise ValueError("normal_depth and flow_fwidth must be (h, w, 4)")
        for arr, shape in ((color_history, (h, w)), (moments_history, (h, w, 4)), (normal_depth_history, (h, w, 4))):
            if arr.dtype != np.float32 or arr.shape != shape or not arr.flags.c_contiguous:
                raise ValueError("history images must be C-contiguous float32 arrays of the viewport's shape")
        out = np.zeros((h, w), dtype=np.float32)
        self._ck(self.L.lv_svgf_denoise_buffers(self.h, w, h, _p(a), _p(nd), _p(ff), _p(color_history), _p(moments_history),
                                                _p(normal_depth_history), _p(out)))
        return out

    def spatial_hashing_denoise(self, noisy, normal_world, position_world, cam_pos):
        """One denoise() of the spatial-hashing denoiser on caller-supplied images (lv_spatial_hashing_denoise_buffers): noisy (h, w),
        normal_world and position_world (h, w, 4), cam_pos (3,).  It accumulates into map 1, which persists across calls.  Returns
        (read, out): the read pass' (h, w) image and the denoised one.  Cell sizes and the map size are the spatial_hashing_* options."""
        a = np.ascontiguousarray(noisy, dtype=np.float32)
        h, w = a.shape
        nm = np.ascontiguousarray(normal_world, dtype=np.float32)
        pm = np.ascontiguousarray(position_world, dtype=np.float32)
        cam = np.ascontiguousarray(cam_pos, dtype=np.float32)
        if nm.shape != (h, w, 4) or pm.shape != (h, w, 4) or cam.shape != (3,):
            raise ValueError("normal_world and position_world must be (h, w, 4), cam_pos (3,)")
        read = np.zeros((h, w), dtype=np.float32)
        out = np.zeros((h, w), dtype=np.float32)
        self._ck(self.L.lv_spatial_hashing_denoise_buffers(self.h, w, h, _p(a), _p(nm), _p(pm), _p(cam), _p(read), _p(out)))
        return read, out

    def spatial_hashing_reset(self, which=0):
        """Empties map `which` (0 = the renderer's, 1 = spatial_hashing_denoise's) and zeroes its statistics."""
        self._ck(self.L.lv_spatial_hashing_reset(self.h, int(which)))

    def spatial_hashing_cells(self, which=0):
        """The occupied cells of map `which` as (keys, sums, counts): uint64 key words (checksum << 32 | hash), the sums of
        floor(100 * occlusion + 0.5) and the contribution counts, in no particular order."""
        n = C.c_uint64(0)
        self._ck(self.L.lv_spatial_hashing_get_cells(self.h, int(which), None, None, 0, C.byref(n)))
        keys = np.zeros(max(n.value, 1), dtype=np.uint64)
        acc = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._ck(self.L.lv_spatial_hashing_get_cells(self.h, int(which), _p(keys), _p(acc), keys.shape[0], C.byref(n)))
        keys, acc = keys[:n.value], acc[:n.value]
        return keys, acc >> np.uint64(28), acc & np.uint64(0x0FFFFFFF)

    def spatial_hashing_stats(self, which=0):
        """{occupied, stored, dropped, clears} of map `which` (lv_spatial_hashing_get_stats)."""
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.L.lv_spatial_hashing_get_stats(self.h, int(which), _p(out)))
        return dict(zip(("occupied", "stored", "dropped", "clears"), (int(v) for v in out)))

    def get_accel(self, num_nodes, num_leaves):
        nodes = np.zeros((max(num_nodes, 1), 16), dtype=np.uint32)
        leaf = np.zeros(max(num_leaves, 1), dtype=np.uint32)
        self._ck(self.L.lv_get_accel(self.h, _p(nodes), nodes.shape[0], _p(leaf), leaf.shape[0]))
        return nodes[:num_nodes], leaf[:num_leaves]
