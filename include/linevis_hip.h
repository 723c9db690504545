/*
 * linevis_hip.h -- C-ABI of the MI355X-native line renderer hot path.
 *
 * Drop-in boundary for chrismile/LineVis' ray-traced line renderers.  The reference has no
 * FFI of its own: its renderers (class LineRenderer, src/Renderers/LineRenderer.hpp:66-277) talk to the GPU through
 * sgl/Vulkan objects.  Each entry point below names the reference interface it replaces; a maintainer binds them
 * from a `LineRenderer` subclass as shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer is a HOST pointer borrowed for the duration of the call unless
 *     the name says `device` (then it is a HIP device pointer, e.g. a torch tensor's data_ptr()).
 *   - return value: LV_OK (0) or a negative LV_E_* code; lv_last_error(ctx) holds a message. No exceptions cross.
 *   - one context = one HIP device = one calling thread at a time (the reference calls every renderer method from
 *     its main thread, src/MainApp.cpp:914-1013).  Multi-GPU = one context per device / process.
 *   - matrices are float32 column-major (GLM layout).  Camera convention owned by the build (sgl::Camera is not
 *     in the reference tree): right-handed view space looking down -z, depth range [0,1], projection with
 *     y flipped so that image row 0 is the top (see linevis_amd/camera.py).
 *   - images are RGBA8, row-major, 4 bytes per pixel, row 0 = top.
 *   - there is NO CPU fallback: every entry point that computes runs hand-written HIP kernels on gfx950 and fails
 *     with LV_E_HIP if no device is present.
 */
#ifndef LINEVIS_HIP_H
#define LINEVIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LV_OK 0
#define LV_E_INVALID (-1)   /* bad argument / unknown option / call order */
#define LV_E_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define LV_E_STATE (-3)     /* missing lines / camera / transfer function / accel */
#define LV_E_CAPACITY (-4)  /* BVH deeper than the traversal stack, buffer too small */

/* RenderingMode ids, src/Renderers/RenderingModes.hpp:32-53 */
/* Deferred shading on a visibility buffer (src/Renderers/Deferred/DeferredRenderer.cpp, "Draw Indexed" with "Precomputed Triangles"):
 * the tube triangle mesh rasterised into one word of primitive index and depth per pixel, every pixel shaded once, opaque; see
 * deferred_rendering_mode, lv_deferred_get_buffers and lv_deferred_shade_buffers below */
#define LV_RENDERING_MODE_DEFERRED_SHADING 1
#define LV_RENDERING_MODE_PER_PIXEL_LINKED_LIST 2
/* Multi-Layer Alpha Blending (src/Renderers/OIT/MLABRenderer.cpp) over the fragments of mode 2's rasterised prism; see
 * mlab_num_layers and lv_mlab_resolve_buffers below */
#define LV_RENDERING_MODE_MLAB 3
/* Depth complexity (src/Renderers/OIT/DepthComplexityRenderer.cpp): the number of fragments of mode 2's rasterised prism per pixel as
 * a colour, and its statistics; see depth_complexity_max_colour, lv_depth_complexity_get_buffers and lv_depth_complexity_get_stats */
#define LV_RENDERING_MODE_DEPTH_COMPLEXITY 5
/* Moment-based order-independent transparency (src/Renderers/OIT/MBOITRenderer.cpp) with power moments stored as float32, over the
 * fragments of mode 2's rasterised prism; see mboit_num_moments and lv_mboit_resolve_buffers below */
#define LV_RENDERING_MODE_MBOIT 6
/* Weighted Blended OIT (src/Renderers/OIT/WBOITRenderer.cpp): the weighted average of all fragments of mode 2's rasterised prism per
 * pixel, in 5 * 8 bytes per pixel; see wboit_depth_weight, lv_wboit_get_buffers and lv_wboit_resolve_buffers below */
#define LV_RENDERING_MODE_WBOIT 8
/* Depth peeling (src/Renderers/OIT/DepthPeelingRenderer.cpp): every fragment layer of mode 2's rasterised prism composited in depth
 * order, exactly, with no fragment storage: memory is bounded by the viewport; see depth_peeling_max_layers,
 * lv_depth_peeling_get_buffers and lv_depth_peeling_resolve_buffers below */
#define LV_RENDERING_MODE_DEPTH_PEELING 9
/* Atomic Loop 64 (src/Renderers/OIT/AtomicLoop64Renderer.cpp): the K nearest fragments of mode 2's rasterised prism per pixel,
 * exactly, in K * 8 bytes per pixel; see atomic_loop_num_layers, lv_atomic_loop_get_buffers and lv_atomic_loop_resolve_buffers below */
#define LV_RENDERING_MODE_ATOMIC_LOOP_64 10
#define LV_RENDERING_MODE_VULKAN_RAY_TRACER 11

/* struct LinePointDataUnified, src/LineData/LineRenderData.hpp:99-106 -- byte-identical (48 B). */
typedef struct lv_line_point {
    float linePosition[3];
    float lineAttribute;
    float lineTangent[3];
    float lineRotation;
    float lineNormal[3];
    uint32_t lineStartIndex;
} lv_line_point;

/* struct TubeTriangleVertexData, src/LineData/LineRenderData.hpp:171-176 -- byte-identical (32 B). */
typedef struct lv_tube_vertex {
    float vertexPosition[3];
    uint32_t vertexLinePointIndex; /* index into the line-point table; bit 31 set on cap vertices */
    float vertexNormal[3];
    float phi;
} lv_tube_vertex;

/* struct HullTriangleVertexData, src/LineData/LineRenderData.hpp:186-191 -- byte-identical (32 B): what lv_set_hull_mesh stores on the
 * device (the paddings are 0). */
typedef struct lv_hull_vertex {
    float vertexPosition[3];
    float padding0;
    float vertexNormal[3];
    float padding1;
} lv_hull_vertex;

/* Counters and timers.  Replaces the per-phase GPU timers of PerPixelLinkedListLineRenderer.cpp:411-420 and the
 * buffer-size reporting of VulkanRayTracer.cpp:671-675.  Ray/node/primitive counters are only filled when the
 * option "collect_stats" is "true" (instrumented kernels; not for timing runs). */
typedef struct lv_stats {
    uint64_t rays_traced;        /* primary + transparency continuation + AO rays */
    uint64_t nodes_visited;      /* 64-byte compressed 4-wide BVH nodes fetched */
    uint64_t prims_tested;       /* 32-byte segment records fetched + capsule tests */
    uint64_t hits_shaded;        /* closest-hit / fragment shading invocations */
    uint64_t fragments;          /* PPLL: value of fragCounter after gather */
    uint64_t ao_hit_pixels;      /* RTAO: pixels whose primary ray hit (compacted list length) */
    uint32_t max_depth_complexity; /* PPLL: longest per-pixel fragment list */
    uint32_t bvh_depth;          /* height of the LBVH */
    uint32_t num_segments;
    uint32_t num_nodes;
    float ms_accel_build;
    float ms_depth_range;
    float ms_ao;                 /* all RTAO kernels of the last lv_render* call */
    float ms_color;              /* ray-tracer colour pass */
    float ms_ppll_clear;
    float ms_ppll_gather;
    float ms_ppll_resolve;
    float ms_total;              /* whole lv_render* call on the stream */
    uint64_t device_bytes;       /* device memory owned by the context */
    /* Per-kernel launch durations from HIP events recorded around every launch on the context's stream, averaged over
     * all launches since lv_reset_timers() (at most the last 512).  Index = LV_KERNEL_*. */
    float ms_kernel_avg[8];
    uint32_t kernel_launches[8];
    /* share of the counters above that belongs to the RTAO sample kernel (k_ao_rays) */
    uint64_t ao_rays_traced;
    uint64_t ao_nodes_visited;
    uint64_t ao_prims_tested;
    /* k_ao_rays lane-utilisation diagnostics (collect_stats only): wave-level iterations and the sum of active lanes
     * of the {refill/setup, node, leaf} phases: utilisation = lanes / (64 * iterations). */
    uint64_t ao_phase_iterations[3];
    uint64_t ao_phase_lanes[3];
    uint32_t max_nodes_per_pixel;  /* collect_stats: most BVH nodes fetched by one pixel of a tile kernel (tail latency) */
    uint32_t num_tube_triangles;   /* triangles of the tube mesh set with lv_set_tube_triangle_mesh */
    uint64_t ppll_pool_nodes;      /* PPLL: physical node slots = linkedListSize + per-wave chunk slack of the gather */
    /* k_ao_rays leaf-test diagnostics (collect_stats only): tests that found a hit inside [0, radius]; tests a
     * conservative axis-distance pre-test would let through; tests axis + bounding-sphere pre-tests would let through */
    uint64_t ao_prim_hits;
    uint64_t ao_prim_may_axis;
    uint64_t ao_prim_may_both;
    /* data set -> first frame on the device (round 6): the triangle LBVH over the tube mesh (its own event pair: ms_accel_build is the
     * segment LBVH only), the device tessellation of lv_set_trajectories' lines (k_tess_*: a14) and the device form of
     * getLinePassTubeAabbRenderData (k_linepoints_*: a2); 0 until the step has run on this context */
    float ms_tri_accel_build;
    float ms_tessellate;
    float ms_line_points;
    uint32_t num_tri_nodes;        /* 64-byte nodes of the triangle LBVH */
    uint32_t tri_leaf_bytes;       /* leaf data per leaf of the triangle LBVH as built: 64 = a pair record (triangle_leaf_records =
                                    * pairs), else 48 x triangle_leaf_size; 0 before the build */
    uint32_t mboit_degenerate_pixels; /* mode 6, collect_stats: pixels with b_0 over the threshold that show the background because
                                       * every fragment's transmittance reconstructed to 0 or NaN (a_sum == 0); one count per
                                       * (tile, pixel) pair of the tile list */
} lv_stats;

#define LV_KERNEL_AO_PRIMARY 0
#define LV_KERNEL_AO_RAYS 1
#define LV_KERNEL_RENDER_RT 2
#define LV_KERNEL_PPLL_GATHER 3
#define LV_KERNEL_PPLL_RESOLVE 4
#define LV_KERNEL_DEPTH_RANGE 5
#define LV_KERNEL_PPLL_SHADE 6   /* fragment stage of ppll_fragment_source = raster_prism (k_ppll_shade_prism) */
#define LV_KERNEL_PPLL_RASTER 7  /* segment rasteriser of raster_prism (k_ppll_raster_prism; ppll_prism_rasteriser = segments) */
/* the simulation-mesh hull pass of modes 5, 8 and 10 (k_hull_pass).  lv_stats' two per-kernel arrays keep their eight entries: this
 * id is read with lv_get_kernel_times and selected with kernel_timers like the others */
#define LV_KERNEL_HULL 8
/* the passes of the spatial-hashing denoiser (ambient_occlusion_denoiser = "Spatial Hashing"), one record per RTAO iteration each:
 * k_sh_write, k_sh_read, and the three a-trous passes of its tail together; read and selected like LV_KERNEL_HULL */
#define LV_KERNEL_SH_WRITE 9
#define LV_KERNEL_SH_READ 10
#define LV_KERNEL_SH_TAIL 11

typedef struct lv_ctx lv_ctx;

/* Renderer construction/destruction: `new VulkanRayTracer(&sceneData, tfWindow)` + initialize(),
 * src/MainApp.cpp:811,840-846. */
lv_ctx* lv_create(int device_ordinal, int* err);
void lv_destroy(lv_ctx* ctx);
const char* lv_last_error(const lv_ctx* ctx);
const char* lv_version(void);

/* Run all kernels of this context on `hip_stream` (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream);
 * NULL selects the context's own stream.  No reference analogue (sgl owns the Vulkan queue). */
int lv_set_stream(lv_ctx* ctx, void* hip_stream);

/* LineRenderer::setLineData(LineDataPtr&, bool) (LineRenderer.hpp:98) fed by
 * LineData::getLinePassTubeAabbRenderData (LineData.hpp:186): 48-byte point records + index pairs, copied to HBM. */
int lv_set_lines(lv_ctx* ctx, const lv_line_point* points, uint32_t num_points,
                 const uint32_t* segment_point_indices /* 2 per segment */, uint32_t num_segments);

/* The triangle tubes the reference's RTAO pass traces against (VulkanRayTracedAmbientOcclusion.cpp:444-445 fetches
 * LineData::getLinePassTubeTriangleMeshRenderData(false, true), LineData.hpp:182): index buffer (3 per triangle),
 * 32-byte TubeTriangleVertexData and the 48-byte line-point table the vertices refer to, copied to HBM.  Belongs to the
 * lines of the last lv_set_lines (a later lv_set_lines drops it); with it the option rtao_geometry = "auto" traces the RTAO rays
 * against these triangles like the reference; the triangle LBVH is built on the next render that needs it. */
int lv_set_tube_triangle_mesh(lv_ctx* ctx, const uint32_t* triangle_indices, uint32_t num_triangles,
                              const lv_tube_vertex* vertices, uint32_t num_vertices,
                              const lv_line_point* line_points, uint32_t num_line_points);

/* The same two inputs WITHOUT the host in between (round 6; band data and helicity: lv_set_trajectories_with_bands):
 * LineDataFlow::setTrajectoryData's arrays (LineDataFlow.cpp:468-578: positions, the selected attribute, one offset per line) are
 * copied to HBM (16 bytes per point) and the device writes what lv_set_lines and lv_set_tube_triangle_mesh would have been handed:
 * the 48-byte line points + index pairs of LineDataFlow::getLinePassTubeAabbRenderData (LineDataFlow.cpp:2112-2277) at once, and the
 * capped triangle tubes of getLinePassTubeTriangleMeshRenderData (LineDataFlow.cpp:1912-2110 -> createCappedTriangleTubesRenderDataCPU,
 * CappedTriangleTubesCPU.cpp:214-383) whenever a frame needs them at a line_width / tube_num_subdivisions they have not been
 * tessellated for -- byte for byte the host layer's output (lv_get_lines / lv_get_tube_triangle_mesh read them back).  A line-width
 * change then costs a tessellation + two LBVH builds on the device instead of seconds on the host and a GB-sized upload.
 * positions: 3 floats per point; attribute: 1 float per point or NULL (zeros); line_offsets: num_lines + 1 non-decreasing entries,
 * [0] = 0.  Replaces the lines and the mesh of earlier lv_set_lines / lv_set_tube_triangle_mesh calls; a later lv_set_lines drops the
 * trajectories, a later lv_set_tube_triangle_mesh overrides the device tessellation until the next lv_set_trajectories. */
int lv_set_trajectories(lv_ctx* ctx, const float* positions, const float* attribute, const uint32_t* line_offsets, uint32_t num_lines);
/* The per-point arrays of band data and of the rotating helicity bands that go to HBM with the trajectories (lv_set_trajectories is
 * lv_set_trajectories_with_bands with bands = NULL).  The records then follow use_ribbons + use_analytic_elliptic_tubes (lineNormal =
 * cross(ribbon direction, tangent), not normalised, LineDataFlow.cpp:2166-2168) and rotating_helicity_bands (lineRotation, a running sum
 * per line, :2188-2197) whenever these options change, and the device mesh follows use_ribbons (the elliptic tubes of band data with
 * semi-axes band_width / 2 * min_band_thickness and band_width / 2) and rotating_helicity_bands (the mesh table's rotation runs on
 * across all lines, :1994,2014-2028).  use_ribbons without ribbon directions, or rotating_helicity_bands without a helicity array,
 * is LV_E_STATE when the geometry is needed. */
typedef struct lv_trajectory_bands {
    const float* ribbon_directions; /* 3 floats per point (LineDataFlow::ribbonsDirections), or NULL */
    const float* helicity;          /* 1 float per point: the helicity attribute (LineDataFlow.cpp:535-550), or NULL */
    float max_helicity;             /* > 0: used as given (LineDataFlow::maxHelicity); <= 0: max |helicity| over all points, reduced on the device */
} lv_trajectory_bands;
int lv_set_trajectories_with_bands(lv_ctx* ctx, const float* positions, const float* attribute, const uint32_t* line_offsets,
                                   uint32_t num_lines, const lv_trajectory_bands* bands);
/* Read-backs of the current line points / index pairs and of the current tube mesh (tessellating it first if lv_set_trajectories'
 * lines have none for the current settings).  Any output pointer may be NULL (query the counts). */
int lv_get_lines(lv_ctx* ctx, lv_line_point* out_points, uint32_t max_points, uint32_t* out_segment_point_indices, uint32_t max_segments,
                 uint32_t* out_num_points, uint32_t* out_num_segments);
int lv_get_tube_triangle_mesh(lv_ctx* ctx, uint32_t* out_triangle_indices, uint32_t max_triangles, lv_tube_vertex* out_vertices,
                              uint32_t max_vertices, lv_line_point* out_line_points, uint32_t max_line_points, uint32_t* out_num_triangles,
                              uint32_t* out_num_vertices, uint32_t* out_num_line_points);

/* Static RTAO prebaking (ambient_occlusion_mode = "RTAO (Prebaker)", VulkanAmbientOcclusionBaker.{hpp,cpp,glsl}): AO
 * factors are baked once per geometry for num_parametrization_vertices points along the lines x
 * rtao_prebaker_num_tube_subdivisions angles and looked up at render time (AmbientOcclusion.glsl:49-75), so AO costs
 * nothing per frame and is view independent.  This call supplies the host-side parametrisation of
 * AmbientOcclusionComputeRenderPass::recomputeStaticParametrization (VulkanAmbientOcclusionBaker.cpp:563-653):
 * blending_weights[i] maps line vertex i (an entry of the mesh's line-point table) to a fractional parametrisation
 * index, sampling_locations[j] is the fractional line-vertex position of parametrisation vertex j.  Baking runs lazily
 * before the next frame (or lv_get_baked_ao) against the triangle tubes set with lv_set_tube_triangle_mesh. */
int lv_set_ao_parametrization(lv_ctx* ctx, const float* blending_weights, uint32_t num_line_vertices,
                              const float* sampling_locations, uint32_t num_parametrization_vertices);
/* The baked table: ambientOcclusionFactors[subdivision + num_tube_subdivisions * parametrization_vertex]. */
int lv_get_baked_ao(lv_ctx* ctx, float* out, uint64_t max_values);
/* Asynchronous baking (the reference's BakingMode::MULTI_THREADED, AmbientOcclusionBaker.hpp:66-73, VulkanAmbientOcclusionBaker.cpp:
 * 266-346: a worker thread bakes while the application keeps rendering and shows the AO once baking has finished).  Here: a second
 * HIP stream with scratch buffers of its own.  lv_bake_ao_start queues the bake and returns; frames rendered meanwhile with
 * ambient_occlusion_mode = "RTAO (Prebaker)" come out WITHOUT ambient occlusion; lv_bake_ao_poll (never blocks) reports whether the
 * bake still runs and whether a valid table is in place -- it and the next lv_render* call adopt a finished table.  Changing anything
 * the table depends on (lines, mesh, parametrisation, line width, baker settings) waits for a running bake and discards its result:
 * start again.  Without lv_bake_ao_start the first frame that needs the table bakes it on the context's stream (synchronously to the
 * stream, as before).  lv_get_baked_ao waits for a started bake. */
int lv_bake_ao_start(lv_ctx* ctx);
int lv_bake_ao_poll(lv_ctx* ctx, int* out_running, int* out_ready);

/* TransferFunctionWindow texture + MinMaxUniformBuffer (Data/Shaders/Utils/TransferFunction.glsl:60-71):
 * n RGBA float texels, sampled with linear filtering at texel centres, clamp-to-edge. */
int lv_set_transfer_function(lv_ctx* ctx, const float* rgba, uint32_t n, float attr_min, float attr_max);

/* LineDataFlow::loadTwistLineTexture (LineDataFlow.cpp:93-171; the "twist_line_texture" file is decoded by the embedder): RGBA8
 * pixels, row-major; sampled with REPEAT addressing at (u, 0.5) where the separator stripes of the rotating helicity bands would be
 * drawn (option use_twist_line_texture = USE_HELICITY_BANDS_TEXTURE, twist_line_texture_filtering_mode[_index] = the six names of
 * LineDataFlow.cpp:55-57; twist_line_texture_max_anisotropy must be 1).  The ray tracer samples level 0 (texture() without
 * derivatives, RayHitCommon.glsl:66-72), the rasterised prism of mode 2 textureGrad with the quad's derivatives of (phi +
 * fragmentRotation) / 2 pi (LinePassGeometryShaderTubes.glsl:724-730).  Texel centres, linear weights, level-of-detail formula and
 * the mip chain (2 x 2 box averages in float) are build-owned.  rgba8 == NULL unloads. */
int lv_set_twist_line_texture(lv_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* SceneData camera + viewport (src/Renderers/SceneData.hpp:49-85) and LineRenderer::onResolutionChanged
 * (LineRenderer.hpp:127); inverses are taken inside as LineData::updateVulkanUniformBuffers does (LineData.cpp:1290-1291).
 * Matrices are float32, column-major (flat index = column * 4 + row).
 *
 * What the kernels' camera arithmetic covers, and the tests exercise (tests/cameras.py):
 *   view  rigid (rotation + translation, any roll, any target, the eye anywhere -- also inside the data set), looking down -z_view;
 *         last row 0 0 0 1.  An affine view that is not rigid is accepted, but distances (depth cues, near / far, AO radius) are then
 *         no longer world distances.
 *   proj  perspective with clip.w = -z_view (last row 0 0 -1 0), depth in 0..1; proj[5] < 0 puts image row 0 at the top (the
 *         convention the frames are compared in).  proj[0] and proj[5] are free: any field of view, and non-square pixels (an aspect
 *         other than width / height).  Lens shift (proj[8], proj[9] != 0: off-centre frusta of tiled and stereo embedders) is covered,
 *         the conservative screen bounds of the sharded PPLL take it into account.  The other entries of rows 0 and 1 are assumed
 *         zero by those bounds.
 *   near_dist / far_dist   the planes proj was built from: fragments of modes 2 / 3 are kept iff near_dist <= -z_view <= far_dist and
 *         the depth range of the depth cues is clamped to them.  far_dist / near_dist up to 1e7 is covered.
 *   fov_y  the vertical field of view proj was built from (halo / outline widths in pixels).
 * LV_E_INVALID, with the previous camera and viewport left in force, for: a non-finite entry or scalar; a view or projection whose
 * determinant is zero, non-finite or below 1e-5 of the product of its column norms (numerically singular); a view whose last row is not
 * 0 0 0 1; a projection whose last row is not 0 0 -1 0 (an orthographic one in particular: rays start at the camera position);
 * near_dist <= 0; far_dist <= near_dist; fov_y outside (0, pi).  A multi-device handle answers for all its ranks. */
int lv_set_camera(lv_ctx* ctx, const float view[16], const float proj[16], float fov_y, float near_dist,
                  float far_dist, uint32_t viewport_width, uint32_t viewport_height);

/* SceneData::clearColor (SceneData.hpp); foreground = 1 - background (LineData.cpp:1282-1283). */
int lv_set_background(lv_ctx* ctx, const float rgba[4]);

/* LineRenderer::setNewSettings(const SettingsMap&) (LineRenderer.hpp:163): same string keys and encodings
 * (InternalState.hpp:43-125; bools are "true"/"1").  Keys:
 *   line_width, depth_cue_strength, ambient_occlusion_mode ("None" | "RTAO (Screen Space)" | "RTAO (Prebaker)"),
 *   ambient_occlusion_strength, ambient_occlusion_gamma              (LineRenderer.cpp:433-498)
 *   ambient_occlusion_iterations, ambient_occlusion_samples_per_frame, ambient_occlusion_radius,
 *   ambient_occlusion_distance_based, use_jittered_primary_rays        (VulkanRayTracedAmbientOcclusion.cpp:115-144)
 *   num_samples_per_frame, num_accumulated_frames (1 = one self-contained frame per lv_render call, the offline default;
 *   N > 1 = the reference's progressive mode: the caller renders frame after frame with the build-owned key frame_number
 *   = 0, 1, ... N-1, every frame is mixed into the previous one THROUGH RGBA8 exactly like TubeRayTracing.glsl:268-273,
 *   and RTAO runs one iteration per frame while frame_number < ambient_occlusion_iterations),
 *   use_deterministic_sampling, geometry_mode ("AABBs (analytic)" = ray-capsule, default | "Triangle Mesh" = the tube
 *   mesh set with lv_set_tube_triangle_mesh | "Linear Swept Spheres" = the capsules with their caps always in the geometry
 *   and the exact roots: what the NVIDIA hardware primitive with chained end caps is, LineData.cpp:909-945),
 *   use_analytic_intersections (bool form of the first two)
 *                                                                       (VulkanRayTracer.cpp:226-278)
 *   use_mlat (multi-layer alpha tracing instead of the transparency loop; either geometry mode), mlat_num_nodes
 *   (power of two in [1, 32], default 8)                                (VulkanRayTracer.cpp:266-275, .hpp:133-134)
 *   mlab_num_layers: numLayers K of rendering mode 3, 1 ... 64 (default 8)  (MLABRenderer.cpp:133-135,330).  Mode 3 folds,
 *   per pixel, the fragments mode 2 keeps (alpha >= 0.001; RTAO, depth cues, band data and rotating helicity bands as in mode 2)
 *   in primitive order -- index-buffer order: segment by segment, triangles 2k, 2k + 1 of a segment -- which is the order of the
 *   reference's default ordered fragment shader interlock; sync modes 0/1/2 of the reference all give this result (primitive
 *   order is one of the orders their races can produce; NO_SYNC's lost updates are not reproduced).  Rules this build owns:
 *   the window depth gl_FragCoord.z is clip.z / clip.w of the fragment's interpolated world position (rows of proj * view in
 *   one fixed float32 order); a pixel whose alphaOut = 1 - transmittance is 0 shows the background (the reference divides 0 / 0).
 *   No fragment is dropped: the fragment pool grows (one host synchronisation per mode-3 frame reads what the rasteriser
 *   needed) and a frame whose pool cannot be allocated, or with a pixel covered by more than 65534 fragments, returns
 *   LV_E_CAPACITY.  ppll_fragment_source = capsule_entry is LV_E_INVALID in mode 3; ppll_max_num_frags and sorting_mode are
 *   ignored; the fold is timed as LV_KERNEL_PPLL_RESOLVE / ms_ppll_resolve.
 *   atomic_loop_num_layers: numLayers K of rendering mode 10, 1 ... 64 (default 8)  (AtomicLoop64Renderer.hpp:112); out of range is
 *   LV_E_INVALID and the old value stays.  Mode 10 keeps, per pixel, the K nearest of the fragments mode 2 keeps (the `kept` rules,
 *   then alpha >= 0.001, AtomicLoop64Gather.glsl:56; RTAO, depth cues, band data and rotating helicity bands as in mode 2) and no
 *   fragment pool.  A fragment is the 64-bit key (window depth bits << 32) | packUnorm4x8(straight colour), compared unsigned -- the
 *   window depth is mode 3's --; a pixel owns K slots, cleared to 0xFFFFFFFFFFFFFFFF.  Insert (AtomicLoop64Gather.glsl:70-79): for
 *   i = 0 ... K - 1: old = atomicMin(slot[i], v); stop if old is the clear value; if old > v then v = old.  Every exchange keeps the
 *   multiset, so the slots end as the K smallest keys in ascending order whatever order the fragments arrive in, and a value still
 *   carried after slot K - 1 is a TAIL fragment.  Rule this build owns: the reference blends a carried colour into
 *   the framebuffer in the order of the racing invocations, which is not defined from run to run; here the tail is order
 *   independent -- five 64-bit integer sums per pixel over the 8-bit channels of the carried keys, SA = sum a8, SR / SG / SB = sum
 *   a8 * r8 / g8 / b8, SL = sum term(a8) with term(0) = 0, term(255) = fixed(1024) and term(a8) = fixed(-log(1 - a8 / 255))
 *   otherwise (the 2^36 fixed point and the log of mode 6).  Tail alpha At = 1 - exp(-unfixed(SL)), tail colour (SR / SA) / 255 per
 *   channel, SA = 0: no tail.  Resolve (AtomicLoop64Resolve.glsl:69-87, float32, one operation at a time): colour = 0, T = 1; per
 *   non-empty slot colour.rgb += (T * a) * rgb, T *= 1 - a; alphaOut = 1 - T; the framebuffer under the layers is the clear colour,
 *   or the tail blended over it (rgb = Ct * At + clear.rgb * (1 - At), a = At + clear.a * (1 - At)); alphaOut > 0: out.rgb = (colour
 *   / alphaOut) * alphaOut + fb.rgb * (1 - alphaOut), out.a = alphaOut + fb.a * (1 - alphaOut), else out = fb.  A pixel with at most
 *   K fragments is the reference's arithmetic bit for bit; frames, tile lists and shards are bit-reproducible.  Memory: (K + 5) * 8
 *   bytes per pixel of the viewport padded to ppll_tile_width x ppll_tile_height plus the two 4-byte per-pixel words of mode 2;
 *   nothing grows with the number of fragments.  One rasteriser launch per frame, no host synchronisation.  The pool options
 *   (ppll_expected_avg_depth_complexity, ppll_max_num_frags, sorting_mode) have no effect; ppll_prism_rasteriser = lbvh,
 *   ppll_fragment_source = capsule_entry and band data with rotating helicity bands return LV_E_INVALID at render time (the
 *   context stays usable).  Statistics: fragments = the fragments past the discard, ppll_pool_nodes = 0.  Timers:
 *   LV_KERNEL_PPLL_RASTER times the pass (with the tile marking and segment culling of a sharded frame), LV_KERNEL_PPLL_RESOLVE
 *   the resolve.  Limit: the sums are exact for up to 131071 kept fragments on a pixel; a pixel with more sets the flag of
 *   mboit_fragment_storage = streamed below, with the same contract (LV_E_CAPACITY from lv_render; the flag stays with the frame
 *   for the asynchronous entry points; a later successful frame clears it).
 *   wboit_depth_weight: "reference" (default) | "opengl": the depth weight of rendering mode 8 (WBOITGather.glsl:21-24); anything
 *   else is LV_E_INVALID and the old value stays; modes other than 8 ignore it.  Mode 8 adds, per pixel, ALL fragments the fragment
 *   stage of mode 2 produces (the `kept` rules only: WBOITGather.glsl has no alpha < 0.001 discard, as mode 6; RTAO, depth cues,
 *   band data and rotating helicity bands as in mode 2) into five sums and keeps no fragment.  Per fragment with the straight colour
 *   (r, g, b, alpha) and the window depth z of mode 3, float32, one operation at a time, left to right: A = min(1, alpha) * 8 +
 *   0.01; B = ((2 * z - 1) * 0.95) - 1 under "reference" (the line the shader runs, with Vulkan's z in [0, 1]) or ((-z) * 0.95) + 1
 *   under "opengl" (the line the shader keeps as a comment); raw = (((((A * A) * A) * 1e8) * B) * B) * B; w = min(max(raw, 0.01),
 *   300), a NaN gives 0.01.  Under "reference" B lies in [-1.95, -0.05], raw is negative and w = 0.01 for every fragment a valid
 *   camera can produce: the reference's frame is the alpha-weighted average of the colours.  Terms, in the
 *   2^-36 fixed point of mode 6 (`fixed`: saturation at +-1024): SR += fixed((r * alpha) * w), SG += fixed((g * alpha) * w), SB +=
 *   fixed((b * alpha) * w), SA += fixed(alpha * w).  Rule this build owns: the reference multiplies 1 - alpha into the revealage in
 *   the blend unit in the order of the racing invocations, and a float product depends on that order; here SL += the term of t = 1 -
 *   alpha: fixed(1024) for t <= 0, 0 for t >= 1 or a NaN, fixed(-log(t)) otherwise (the log of mode 6), and the revealage is R =
 *   exp(-unfixed(SL)).  All sums are 64-bit integers: any order and any split of the fragments gives the same bits.  Resolve
 *   (WBOITResolve.glsl:38-48, then BACK_TO_FRONT_STRAIGHT_ALPHA over the clear colour): a pixel without fragments or with R > 0.9999
 *   is the clear colour; otherwise c = unfixed(S) / max(unfixed(SA), 1e-5) per channel, a = 1 - R, out.rgb = c * a + clear.rgb * (1
 *   - a), out.a = a + clear.a * (1 - a), stored as RGBA8 like every frame.  (The shader's isinf branch cannot be reached: the terms
 *   saturate.)  Memory: 5 * 8 bytes per pixel of the viewport padded to ppll_tile_width x ppll_tile_height plus the two 4-byte
 *   per-pixel words of mode 2; nothing grows with the number of fragments.  One rasteriser launch per frame, no host
 *   synchronisation.  The pool options (ppll_expected_avg_depth_complexity, ppll_max_num_frags, sorting_mode) have no effect;
 *   ppll_prism_rasteriser = lbvh, ppll_fragment_source = capsule_entry and band data with rotating helicity bands return
 *   LV_E_INVALID at render time (the context stays usable).  Statistics: fragments = the kept fragments, ppll_pool_nodes = 0,
 *   max_depth_complexity.  Timers: LV_KERNEL_PPLL_RASTER times the pass (with the tile marking and segment culling of a sharded
 *   frame), LV_KERNEL_PPLL_RESOLVE the resolve.  Limit: the sums are exact for up to 131071 kept fragments on a pixel; a pixel with
 *   more sets the flag of mboit_fragment_storage = streamed below, with mode 10's contract.
 *   depth_peeling_max_layers: 1 ... 2000 (default 2000, the reference's constant, DepthPeelingRenderer.cpp:288): the cap of rendering
 *   mode 9's passes; anything else is LV_E_INVALID and the old value stays; modes other than 9 ignore it.  Mode 9 peels, per pixel,
 *   the fragments mode 8 adds (the `kept` rules only, no alpha discard; RTAO, depth cues, band data and rotating helicity bands as in
 *   mode 2) layer by layer in depth order.  Per fragment: the straight float32 colour c, the window depth z of mode 3 and the
 *   primitive key k of mode 3 (segment << 6 | triangle: index-buffer order).  The frame first counts the fragments per pixel (as mode
 *   5) and reads the maximum D back: the frame's one host synchronisation, the reference's syncWithCpu; with lv_create_multi it
 *   serialises the ranks' front ends as mode 3's does.  Then min(D, depth_peeling_max_layers) passes.  Pass i takes, per pixel, what
 *   DepthPeelingGather.glsl:42-49 and the depth test leave (cleared to 1.0, LESS, depth write on): the fragment with the smallest z
 *   that is > the previous layer's z (any z in pass 0) and < 1.0; among fragments of equal z the smallest k.  A fragment with z >=
 *   1.0 (or a z whose sign bit is set) is never peeled; fragments that share a depth with a peeled one are never peeled later.  The
 *   layer's colour s = (c.rgb * c.a, c.a) goes into the accumulator A (cleared to 0) with FRONT_TO_BACK_PREMUL_ALPHA, float32,
 *   unfused: t = 1 - A.a; A.x = A.x + s.x * t for x in r, g, b, a, all four with the old A.a.  After the last pass out = A + clear *
 *   (1 - A.a) on all four channels (BACK_TO_FRONT_PREMUL_ALPHA), stored as RGBA8 like every frame.  The passes do not shade: the
 *   discard depends on the depth only, so a pass is the rasteriser plus the position of every kept fragment and one 64-bit atomicMin
 *   on (bits(z) << 32 | k); the winner of every pixel is shaded once, afterwards.  Memory: 32 bytes per pixel of the viewport padded
 *   to ppll_tile_width x ppll_tile_height plus the two 4-byte per-pixel words of mode 2; nothing grows with the number of fragments.
 *   The pool options have no effect; ppll_prism_rasteriser = lbvh, ppll_fragment_source = capsule_entry and band data with rotating
 *   helicity bands return LV_E_INVALID at render time (the context stays usable).  Statistics: fragments = the kept fragments,
 *   ppll_pool_nodes = 0, max_depth_complexity.  Timers: LV_KERNEL_PPLL_RASTER times the count pass (with the tile marking and
 *   segment culling of a sharded frame) and then every peel pass, LV_KERNEL_PPLL_GATHER the reduction of the counts,
 *   LV_KERNEL_PPLL_SHADE the layer launches, LV_KERNEL_PPLL_RESOLVE the blit.
 *   hull_opacity: 0 ... 1 (LineData.cpp:142-145): the opacity of the simulation-mesh hull (lv_set_hull_mesh).  The hull is drawn iff a
 *   mesh is set AND this key has been set to a value > 0 -- the reference's shallRenderSimulationMeshBoundary, false until the
 *   setting arrives; the value in force before any set is 0.3 (LineData.hpp:474) and draws nothing.
 *   hull_color: three floats "r g b" (blanks or commas between them), linear RGB, each 0 ... 1.  Default: the linear value of sRGB 0.5
 *   by the standard piecewise formula, ((0.5 + 0.055) / 1.055)^2.4 evaluated in double = 0.21404114048223255, as float32
 *   0.214041144 (bits 0x3E5B2D9A), three times (LineData.hpp:472-473).
 *   hull_use_shading: "true" | "1" | "false" | "0", default true (LineData.hpp:475): blinnPhongShading(hullColor, normal) of
 *   Lighting.glsl:45-92 under MESH_HULL, else the plain hull_color.
 *   What draws the hull: rendering modes 5, 8 and 10, between the mode's line pass and its resolve -- every hull fragment is one
 *   more fragment of the pixel (coverage and depth by mode 1's rules with culling off, alpha = hull_opacity * (1 - |normal . v|) with
 *   the interpolated normal NOT normalised, MeshHull.glsl:77-90; mode 10 discards alpha < 0.001, modes 8 and 5 discard nothing), so
 *   mode 5's counts, maximum and statistics, mode 8's sums and counts and mode 10's slots, tail and counts include it; memory added
 *   to a frame: none beyond the mesh; timer: LV_KERNEL_HULL.  Modes 6 and 9 draw no hull in the reference (MBOITRenderer.cpp:84 and
 *   DepthPeelingRenderer.cpp:86 reset the pass) and none here: they render the same frame with or without a mesh.  Modes 1, 2, 3
 *   and 11 are not built for the hull: while a hull would be drawn lv_render returns LV_E_INVALID for them (the message names modes
 *   5, 8 and 10; the context stays usable); with hull_opacity 0 or no mesh they render as without these keys, byte for byte.  Two
 *   build-owned switches, below, lift the refusal: hull_fragment_pool = on for modes 2 and 3, hull_ray_tracing = on for mode 11.
 *   hull_ray_tracing (build-owned switch): "off" (default: everything above, the refusal of mode 11 included) | "on": a mode-11
 *   frame draws the hull while one is drawn by the rule of hull_opacity -- the reference puts a hull triangle BLAS into every TLAS of
 *   the ray tracer (LineData.cpp:949-1162) and shades its hits in ClosestHitHull (TubeRayTracing.glsl:359-431) inside the transparency
 *   loop of the lines.  Per step of that loop the nearer of the closest line hit and the closest hull hit is taken (a tie goes to the
 *   line); the hull hit is the least t over the triangles the build's ray-triangle test accepts (Moeller-Trumbore without culling +
 *   the own-box rule with pad = maxAbs * 1e-5 + 1e-6, maxAbs = the mesh's largest absolute coordinate; ties: lowest triangle index),
 *   shaded with the interpolated normal NORMALISED (alpha = hull_opacity * (1 - |n . v|)), payload.hitT = |position - camera|; the
 *   semantics are stated once in csrc/lv_hull_rt.h.  The colour pass is then k_render_rt_hull, for every geometry mode and band
 *   variant of the colour pass (not under shading_numerics = fast, which is refused: see rt_record_hits); the hull's LBVH is built
 *   by the first frame or lv_trace_rays_hull call that needs it, rebuilt after lv_set_hull_mesh and by nothing else.  With "on" and
 *   no hull drawn the frame is the "off" frame byte for byte (the same kernels run).  use_mlat together with a drawn, ray-traced hull
 *   returns LV_E_INVALID (the any-hit variant AnyHitHull is not built); modes 1, 2 and 3 keep refusing.
 *   hull_fragment_pool (build-owned switch): "off" (default: everything above, the refusal of modes 2 and 3 and its message
 *   included) | "on": a mode-2 or mode-3 frame draws the hull while one is drawn by the rule of hull_opacity -- the reference draws
 *   it inside the gather of its pooled renderers (PerPixelLinkedListLineRenderer.cpp:448-461), after the lines, through the same
 *   gatherFragment.  The hull fragment is the one above (coverage, 0 <= z < 1, position, normal, colour); alpha < 0.001 is
 *   discarded by both gathers.  Mode 2: the node {packed straight colour, bits of |position - camera|} is sorted and blended with
 *   the line nodes, takes a slot of the same pool (dropped like a line fragment where the pool is full) and is exported by
 *   lv_ppll_get_buffers like any node.  The hull's slots are taken BEFORE the lines' (its ranks come first in every run), so a
 *   mode-2 frame whose pool runs full drops line fragments first -- the reference draws the hull last and would drop hull fragments
 *   first; either frame is one its pool cannot hold, raise ppll_expected_avg_depth_complexity.  Mode 3: the entry {packUnorm4x8(rgb
 *   * a, 1 - a), window depth, key} with key = (segments << 6) + hull triangle folds after every line fragment of its pixel, in
 *   triangle order (the reference's ordered interlock: the hull is drawn after the lines); (segments << 6) + hull triangles >
 *   0xFFFFFFFE returns LV_E_INVALID.  Both: a stored hull fragment counts in the pixel's 16-bit count (a pixel holds at most 65535
 *   fragments, lines and hull together: mode 2 drops the rest, mode 3 returns LV_E_CAPACITY), a kept one in lv_stats.fragments;
 *   tile lists, shards and lv_create_multi handles as for the lines.  Memory added: 4 bytes per pixel of the padded viewport, and
 *   pool slack for the hull launch's waves; no host synchronisation added; timer: LV_KERNEL_HULL (two launches per frame).  While a
 *   hull is drawn under "on", ppll_prism_rasteriser = lbvh, ppll_fragment_source = capsule_entry and line_primitive_mode = "Quads
 *   (Programmable Pull)" return LV_E_INVALID at render time: the hull is stored in the segment rasteriser's pool only.  Pooled mode
 *   6 draws no hull, modes 1 and 11 are untouched by this switch; with "on" and no hull drawn every frame is the "off" frame byte
 *   for byte.  The semantics are stated once in csrc/lv_hull_pool.h.
 *   rt_record_hits (build-owned: "true" | "1" | "false" | "0", default false) / rt_hits_capacity (records, default 4 Mi, at most
 *   64 Mi): a mode-11 frame without use_mlat runs k_render_rt_hull -- also when no hull is drawn -- and records every step of every
 *   pixel's loop for lv_rt_get_hits.  A record numbers the steps of a loop in 16 bits: a recording frame with max_depth_complexity
 *   above 65536 returns LV_E_INVALID.  k_render_rt_hull has no variant for shading_numerics = fast: a frame it would render -- a
 *   recording frame, or a frame with a drawn, ray-traced hull -- returns LV_E_INVALID under that option instead of a frame with
 *   other lighting than the non-recording one (the message names shading_numerics).
 *   line_primitive_mode: "Tube (Programmable Pull)" (default: the programmable-pull N-gon prism, today's frames byte for byte) |
 *   "Quads (Programmable Pull)" (LineData::LinePrimitiveMode by its display name, LineData.cpp:56-74; LinePassQuads.glsl): two
 *   camera-facing triangles per segment, shaded as a round tube from one interpolated coordinate.  Every other name of the reference's
 *   list ("Quads (Geometry Shader)", "Tube (Geometry Shader)", "Tube (Triangle Mesh)", the mesh-shader and ribbon modes) is
 *   LV_E_INVALID with a message that says the mode is not built, and the old value stays.  While quads are selected: rendering modes
 *   5, 8 and 10 draw their line pass with quads (the hull pass, tile lists, shards and lv_create_multi handles as before; RTAO (Screen
 *   Space) and depth cues are supported); modes 2, 3, 6 and 9 return LV_E_INVALID (the message names modes 5, 8 and 10; the context
 *   stays usable); modes 1 and 11 ignore the option, as the reference, which never reads linePrimitiveMode there.  With quads,
 *   LV_E_INVALID also for use_ribbons, rotating_helicity_bands, ambient_occlusion_mode = "RTAO (Prebaker)" (its lookup needs
 *   phi = asin(x)), ppll_fragment_source = capsule_entry and ppll_prism_rasteriser = lbvh.  shading_numerics = fast: quads are shaded
 *   by the exact path.  Build-owned definitions: line point i yields vertex 2 i (shiftSign -1) and 2 i + 1 (+1) at
 *   linePoint + ((shiftSign * lineWidth) * 0.5) * offsetDirection, offsetDirection = normalize(cross(normalize(cameraPosition -
 *   linePoint), normalize(tangent))), in float32 with the shading code's normalize; triangles (2a, 2b, 2b + 1), (2a, 2b + 1, 2a + 1);
 *   coverage, fill rule, perspective-correct weights and the three kept rules are the prism's; a quad is front-facing by construction,
 *   only the flipped triangle of a bow-tie is culled; a point whose tangent is parallel to its view direction gets a zero offset (the
 *   shading code's normalize of a zero vector is zero, not NaN): a line seen exactly end-on draws nothing, and no colour is NaN.  Where GLSL
 *   leaves asin / sin / cos to the driver the normal is xc = clamp(x, -1, 1), fragmentNormal = sqrt(fma(-xc, xc, 1)) *
 *   normalize(normal0) + xc * normalize(normal1); EPSILON_WHITE = fwidth(|x|) comes from the 2 x 2 partners' rays on the same
 *   triangle.  Timer: the quads pass is what LV_KERNEL_PPLL_RASTER times in these frames.
 *   deferred_rendering_mode: "Draw Indexed" (the reference's default, DeferredRenderer.hpp:297) only; draw_indexed_geometry_mode:
 *   "Precomputed Triangles" (:300) only; supersampling: 1 only.  The other values the reference knows ("Draw Indirect", "Task/Mesh
 *   Shader", "BVH Draw Indirect", "BVH Mesh Shader"; "Programmable Pulling"; 2, 4, 8 ...) are LV_E_INVALID with a message that says the
 *   value is not built, and the old value stays; modes other than 1 ignore the three.  Mode 1 works on the context's tube triangle
 *   mesh (lv_set_tube_triangle_mesh, or the device tessellation of lv_set_trajectories[_with_bands], tessellated first if stale);
 *   without one lv_render returns LV_E_STATE.  Pass 1, the visibility buffer: one 64-bit word per pixel, (bits(z) << 32) | primitive
 *   index, empty = (bits(1.0) << 32) | 0xFFFFFFFF (depth clear 1.0, primitive clear 0xFFFFFFFF, DeferredShading.glsl:73); every
 *   covered, kept fragment is one atomicMin: depth test LESS, the first primitive in index-buffer order among equal depths.  The
 *   rules the reference leaves to the driver are the build's: coverage is decided on the pixel-centre viewing ray (the coverage
 *   direction D of mode 2's prism, its basis P = cross(right, D), Q = cross(D, P); a vertex is (A . P, A . Q) with A = position -
 *   camera, unfused; edge function E(U, V) = yU * xV - xU * yV, unfused, so E(V, U) = -E(U, V) bit for bit; covered iff E(V1, V2),
 *   E(V2, V0), E(V0, V1) and their sum are > 0, an edge with E == 0 belonging to the triangle that runs through it with ascending
 *   vertex index); FRONT is det = A0 . cross(A1 - A0, A2 - A0) < 0, the sense of the tessellator's outward triangles, det == 0 covers
 *   nothing, back faces are culled iff use_capped_tubes (VisibilityBufferDrawIndexedPass.cpp:77-81) and otherwise covered with the
 *   signs reversed; a triangle that crosses the near plane is not clipped; z = clip.z / clip.w (rows of projection * view as mode 3's
 *   window depth) of the perspective-correct position sum(b_i V_i), b_i = E_i * (1 / sum E); kept iff 0 <= z < 1 (a z whose sign bit
 *   is set is refused).  Pass 2 shades every pixel once (DeferredShading.glsl:90-134): an empty word is the background colour; else
 *   the position from the pixel centre and z through the inverse matrices, (u, v, 1 - u - v) from cross-product areas,
 *   LineAttributesBarycentric.glsl (isCap, interpolateAngle, the helicity cap continuation), computeFragmentColor with
 *   fragmentColor.a = 1, the AO texel the pixel's own; the screen-space RTAO, depth cues, band data (use_ribbons) and rotating
 *   helicity bands as in mode 11's "Triangle Mesh".  The prebaked AO table is not built for this pass: lv_render returns
 *   LV_E_INVALID with it (the context stays usable).  A triangle with a vertex at clip w <= 0 is tested against every pixel of the
 *   viewport (64 pixels per wave step).  No host synchronisation, no pool; memory: 8 bytes per pixel of the viewport padded to ppll_tile_width x
 *   ppll_tile_height plus mode 2's 4-byte mask word.  A rank of a sharded frame walks all triangles.  Statistics: fragments = the
 *   requested pixels with a winner.  Timers: LV_KERNEL_PPLL_RASTER times the visibility pass (with its clear and the tile marking of a
 *   sharded frame), LV_KERNEL_PPLL_RESOLVE the shading pass.  Not built: "Programmable Pulling" geometry, the Draw Indirect, BVH and
 *   mesh-shader modes, HZB culling, meshlets, supersampling and upscalers, motion vectors, the hull pass, stress-line data, per-rank
 *   triangle culling for sharded frames.
 *   depth_complexity_max_colour: 0 (default) ... 1000000: numFragmentsMaxColor of rendering mode 5; anything else is LV_E_INVALID and
 *   the old value stays; modes other than 5 ignore it.  Mode 5 counts, per pixel, the fragments mode 8 adds (n) and shows percentage =
 *   clamp(float(n) / float(min(numFragmentsMaxColor, 512)), 0, 1) (DepthComplexityResolve.glsl:48-57) as the colour (0, 1, 1,
 *   percentage) blended over the clear colour: out.rgb = colour.rgb * percentage + clear.rgb * (1 - percentage), out.a = percentage +
 *   clear.a * (1 - percentage) (BACK_TO_FRONT_STRAIGHT_ALPHA), float32, unfused.  0 = auto: numFragmentsMaxColor = uint32(float(max(
 *   maxComplexity, 4)) / 1.5f) (DepthComplexityRenderer.cpp:332).  Rule this build owns: the reference takes maxComplexity from a
 *   statistics read-back that lags by up to a second; here it is the maximum over THIS frame's requested pixels, computed on the
 *   device and read by the resolve from device memory: a mode-5 frame has no host synchronisation.  A tile list or a shard of a
 *   multi-device frame sees only its own pixels' maximum, so only an explicit value makes them reproduce the whole frame.  The
 *   restrictions, memory (without the 32 bytes) and statistics of mode 9; timers: LV_KERNEL_PPLL_RASTER the count pass,
 *   LV_KERNEL_PPLL_GATHER the reduction, LV_KERNEL_PPLL_RESOLVE the resolve.
 *   mboit_num_moments: 4 | 6 | 8 power moments of rendering mode 6 (default 4)   (MBOITRenderer.cpp:41-45).  Mode 6 sweeps, per
 *   pixel, ALL fragments the fragment stage of mode 2 produces (the alpha < 0.001 discard of modes 2 and 3 is not MBOIT's; its own
 *   rules are transmittance > 0.9999999 per fragment in the moment pass and b_0 < 0.00100050033 per pixel) twice: power moments of
 *   the absorbance over the log-warped view depth, then per fragment the reconstructed transmittance and the colour sums, then the
 *   blend over the background.  Rules this build owns: the view depth is row z of the view matrix applied to the
 *   fragment's interpolated world position in one fixed float32 order; the log depth range is computed from the eight corners of
 *   the line points' box with the build's log; per-pixel sums are sums of 64-bit fixed-point terms rint(term * 2^36) (|term|
 *   saturates at 1024), so the frame does not depend on the order of the fragments; log / exp / atan2 / sin / cos are the build's
 *   fixed float32 definitions and fma() is fused; a pixel whose colour weight sum is 0 although b_0 is over the threshold (the
 *   reconstruction degenerated: typically a single fragment with the default bias) shows the background and is counted in
 *   lv_stats.mboit_degenerate_pixels.  Pool, LV_E_CAPACITY, capsule_entry and the timer slot as mlab_num_layers above.
 *   mboit_overestimation: overestimationBeta in [0, 1] (default 0.1)    (MBOITRenderer.cpp:45,609)
 *   mboit_moment_bias: "auto" (default; 5e-7 / 5e-6 / 5e-5 for 4 / 6 / 8 moments, MBOITRenderer.cpp:136-145) or a float in (0, 0.1]
 *   mboit_use_power_moments ("true" only), mboit_pixel_format ("Float" only): trigonometric moments and the 16-bit quantised
 *   storage are not built; "false" / "UNORM" return LV_E_INVALID
 *   mboit_fragment_storage: "pool" (default) | "streamed"; any other value is LV_E_INVALID and leaves the old value in force; modes
 *   other than 6 ignore it.  "streamed" keeps no fragment pool: as the reference's MBOITRenderer the frame rasterises and shades
 *   the geometry twice and accumulates per pixel with 64-bit integer atomics on the fixed-point terms above -- first the moment
 *   sums, then the colour sums --, then blends.  The frame, the statistics and lv_mboit_get_moments equal the pooled frame's bit
 *   for bit (same terms, integer addition).  Memory: (1 + N + 4) * 8 bytes of accumulators per pixel of the viewport padded to
 *   ppll_tile_width x ppll_tile_height, plus the two 4-byte per-pixel words of mode 2; nothing grows with the number of
 *   fragments (the pool costs 12 + 20 = 32 bytes per fragment: break-even at 2.25 / 2.75 / 3.25 fragments per pixel for N = 4 /
 *   6 / 8).  The pool options ppll_expected_avg_depth_complexity, ppll_max_num_frags and sorting_mode have no effect.  No host
 *   synchronisation per frame and no second run of the front end; the line points' box is read back once per acceleration
 *   structure build.  ppll_prism_rasteriser = lbvh and ppll_fragment_source = capsule_entry return LV_E_INVALID at render time
 *   (the context stays usable).  Statistics (collect_stats): every counter of lv_get_stats equals the pooled frame's except
 *   ppll_pool_nodes (0) and device_bytes; rays_traced, prims_tested, hits_shaded and fragments are counted in the moments pass
 *   only.  Timers: LV_KERNEL_PPLL_RASTER times the two pass launches (2 launches per frame, the first with the tile marking and
 *   segment culling of a sharded frame), LV_KERNEL_PPLL_RESOLVE the blend, LV_KERNEL_PPLL_SHADE has no launch.  Limit: the
 *   per-pixel count is 32 bits and the sums are exact for up to 2^63 / (1024 * 2^36) = 131071 kept fragments on a pixel (the
 *   pool's limit is 65534); the blend flags a pixel with more.  lv_render reads the flag with the frame and returns
 *   LV_E_CAPACITY; lv_render_device / lv_render_tiles_device stay asynchronous and the flag stays with the frame: the next
 *   host-synchronous call that reads anything of that frame -- lv_get_stats, lv_mboit_get_moments -- returns LV_E_CAPACITY.  A
 *   later successful frame clears it.
 *   use_capped_tubes, use_halos, tube_num_subdivisions                  (LineData.cpp:87-181)
 *   max_depth_complexity                                                (VulkanRayTracer.hpp:139)
 *   ppll_max_num_frags, ppll_expected_avg_depth_complexity, ppll_tile_width, ppll_tile_height
 *                                                                       (PerPixelLinkedListLineRenderer.cpp:144-209,251-357)
 *   sorting_mode: the "Sorting Mode" combo box of the PPLL renderer (.cpp:470-475, GUI-only in the reference): a name of
 *   SORTING_MODE_NAMES -- "Priority Queue" (default) | "Bubble Sort" | "Insertion Sort" | "Shell Sort" | "Max Heap" |
 *   "Bitonic Sort" | "Quicksort" | "Quicksort Hybrid" (src/Renderers/PPLL.hpp:32-50) -- or its index 0..7,
 *   accel_build (build-owned; the reference builds its BLAS with VK_BUILD_ACCELERATION_STRUCTURE_PREFER_FAST_TRACE_BIT_KHR,
 *   LineData.cpp:740-741): "fast_trace" (default: LBVH whose subtrees of <= treelet_leaves leaves are rebuilt with a binned
 *   surface-area heuristic) | "fast_build" (the plain LBVH); treelet_leaves (3 ... 4096, default 512),
 *   accel_partition (fast_trace only): "sah" (default: a binned-SAH partition of the whole scene chooses the leaf sets of the
 *   treelets -- path-code bits in front of the Morton sort keys) | "morton" (runs of the Morton order do); same hits either way; accel_partition_min_leaves
 *   (default 65536; 0 = always): builds of fewer leaves keep the Morton order under "sah" too,
 *   treelet_group_leaves (0 | 8 | 16, default 16), treelet_lane_leaves (0 | 2 ... 64, default 6; used when the former is 0),
 *   treelet_plane_eval ("scan" | "loop"), accel_collapse_top ("true" | "false"): build time only, the tree is the same -- the
 *   small ranges of a treelet are built by groups of 8 / 16 lanes (or one lane per range) instead of by the whole wave; the form
 *   of the wave's plane evaluation; the top levels of the 4-wide collapse in one launch,
 *   kernel_timers (build-owned): "all" (default) | "none" | comma-separated LV_KERNEL_* numbers and / or "phases" -- which launches
 *   of a frame are bracketed by HIP events (lv_get_kernel_times; "phases": the ms_* fields of lv_get_stats, 0 otherwise).  An event
 *   record costs the stream 2 - 4 us: a frame with every kernel and phase bracketed carries a dozen (6 % of a 0.8-ms PPLL frame),
 *   triangle_leaf_size (build-owned): consecutive triangles per leaf of the triangle LBVH, 1 ... 8 (default 2: a tube face);
 *   changes the acceleration structure only, never a hit,
 *   triangle_leaf_records (build-owned): "pairs" (default) | "triangles" -- with two triangles per leaf and a mesh in which the
 *   second triangle of every leaf has at most one vertex index the first one lacks (every mesh the tessellator writes: tube faces,
 *   cap quads, fan pairs), a leaf stores the four vertices once (64 B) instead of two 48-B triangle records; the ray-triangle test
 *   runs on the same operands in the same order, so no hit changes; other meshes and "triangles" keep the 48-B records,
 *   shading_numerics (build-owned): "exact" (default: every operation of the shading code in IEEE float32 with one fixed evaluation
 *   order -- frames, AO factors and PPLL fragments are bit-identical to the CPU checker's) | "fast": the hardware's approximate
 *   reciprocal square root / reciprocal / log2 / exp2 (<= 1 ulp) in arithmetic that only reaches a COLOUR -- the normalisations,
 *   pow() and divisions of blinnPhongShadingTube (Lighting.glsl:100-191) and, in the raster colour of plain tubes, of the halo
 *   coordinate (LinePassGeometryShaderTubes.glsl:732-1129).  Hits, coverage, fragment depths, alpha values, list lengths and the
 *   RTAO factors stay bit-identical; colours move by <= 1 LSB, the contract is +- 2 LSB.  Applies to the ray tracer's capsule colour
 *   pass and the rasterised prism's fragment stage of plain flow lines; all other variants keep the exact arithmetic,
 *   overlap_primary_passes (build-owned; "auto" (default) | "true" | "false"): in a ray-tracer frame with per-frame RTAO the closest hits of the colour
 *   pass' rays do not depend on the AO image, only their shading does -- they are traced in ONE launch with the RTAO pass' primary
 *   rays (two latency-bound passes that a rank owning 1/8 of the tiles cannot fill the GPU with one after the other) and the colour
 *   kernel after the RTAO pass shades them; "false" = one pass after the other as in VulkanRayTracer::render (VulkanRayTracer.cpp:
 *   131-154); "auto" = overlapped while the tile list is at most half a 1920 x 1080 frame (a sharded frame's rank), one after the
 *   other for a whole frame on one GPU, where both passes are throughput-bound.  The frame is byte-identical either way,
 *   ao_ray_generation (build-owned, no counterpart): "per_pixel" (default: with ambient_occlusion_samples_per_frame a multiple of 64 a
 *   batch of 64 AO rays is 64 samples of one pixel, and the sample kernel looks that pixel up once per batch) | "per_ray" (every ray
 *   looks its pixel up; always the path of other sample counts, of collect_stats and of the prebaker); the AO image is bit-identical,
 *   traversal_reciprocal (build-owned, no counterpart; lv_trace_rays and lv_trace_rays_triangles only): "ieee" (default) | "hardware" =
 *   the node steps of these two entry points use the hardware reciprocal of the direction, as the RTAO sample kernel always does; the
 *   hits are bit-identical (the slab test's margins cover the <= 1 ulp; leaf tests divide by IEEE rules) -- a way to put arbitrary rays,
 *   axis-parallel and denormal directions among them, through that arithmetic,
 *   dispatch_order (build-owned, no counterpart): "cost" (default: the tile kernels start their 64x64-pixel groups heaviest-of-
 *   the-previous-frame first, see lv_get_dispatch_order) | "as_numbered" (tile-list order); the image is the same,
 *   rtao_prebaker_iterations (128), rtao_prebaker_samples_per_frame (4), rtao_prebaker_num_tube_subdivisions (8): the
 *   prebaker's settings, GUI-only in the reference (VulkanAmbientOcclusionBaker.hpp:108,165-166); radius / distance
 *   based use the ambient_occlusion_* keys,
 *   collect_stats (build-owned: run the instrumented kernels), mlat_record_trace / mlat_trace_capacity (build-owned,
 *   with collect_stats: record the candidate visiting order of an MLAT frame for lv_get_mlat_trace; records, 4 Mi),
 *   rtao_geometry (build-owned): "auto" (default: "triangle_tubes" -- the only geometry the reference's RTAO pass traces,
 *   VulkanRayTracedAmbientOcclusion.cpp:437-456 -- once lv_set_tube_triangle_mesh has been called for the current lines,
 *   "capsules" before that) | "triangle_tubes" (fails without the mesh) | "capsules" (AO rays hit the analytic capsules of the
 *   colour pass: not a mode of the reference),
 *   intersection_form (build-owned): "auto" (default: "literal", the reference's formula, in every frame the reference can
 *   render; "closest_approach" only where the RTAO rays of the frame are traced against the analytic capsules, a mode the
 *   reference does not have -- rays that start on a capsule need the stable roots) |
 *   "literal" (the reference's textbook roots, RayIntersectionTestsVulkan.glsl:39-119, with the own-box rule that keeps them
 *   independent of the BVH) | "closest_approach" (the same roots evaluated stably: NOT the reference's formula),
 *   ppll_fragment_colour (build-owned): "raster" (default: the PPLL gather shades with the raster tube shader's variant of
 *   computeFragmentColor, LinePassGeometryShaderTubes.glsl:785-815,1079-1087 -- EPSILON_OUTLINE = 0, EPSILON_WHITE =
 *   fwidth(ribbonPosition) over the 2 x 2 pixel quad, cap halo min(rp, |rp2|)) | "ray_tracer" (RayHitCommon.glsl's, a probe),
 *   ppll_fragment_source (build-owned): "raster_prism" -- the fragments of mode 2 are those of the geometry the reference
 *   RASTERISES in its default "Tube (Programmable Pull)" mode: per segment the uncapped N-gon prism (N = tube_num_subdivisions) of
 *   LinePassProgrammablePullTubes.glsl:87-224 / LineDataFlow.cpp:1698-1713, back faces culled (LineRasterPass.cpp:85-96), the
 *   fragment shader fed with perspective-correct interpolated position / normal / tangent / attribute; the rasteriser is a
 *   watertight edge-function rasteriser in the space of the pixel's viewing ray (linevis_amd/csrc/lv_prism.h) | "capsule_entry"
 *   -- entry hits of the pixel-centre ray against the analytic capsules / elliptic tubelets (rounds 1-3 of this build; a probe) |
 *   "auto" (default: raster_prism wherever its fragment stage is built -- plain flow lines and band data, whose prism is the
 *   elliptic ring of the USE_BANDS vertex stage, LinePassProgrammablePullTubes.glsl:112-116,166-171, radius band_width / 2,
 *   shaded by the band branch of the raster fragment shader, and the rotating helicity bands (interpolated phi / fragmentRotation,
 *   UNIFORM_HELICITY_BAND_WIDTH from the line points around floor(fragmentVertexId), LinePassGeometryShaderTubes.glsl:1017-1052);
 *   capsule_entry for band data with helicity bands),
 *   ppll_prism_rasteriser (build-owned): front end of raster_prism -- "segments" (default: one lane per line segment over the
 *   screen rectangle of its ring vertices, like the hardware the reference draws with walks primitives, not pixels) | "lbvh"
 *   (the all-hits walk of the viewing rays through the segment LBVH); both decide every (pixel, segment) pair by the same
 *   coverage test and produce the same fragments.  The ORDER of a pixel's fragments is not defined (the reference's fragment
 *   shader invocations race for the list heads, LinkedListGather.glsl:55); where a pixel keeps more fragments than
 *   ppll_max_num_frags, this build resolves the NEAREST ones by the (depth, colour) key (one of the subsets the reference's
 *   race can leave in the first MAX_NUM_FRAGS nodes), so frames do not depend on that order; lv_ppll_get_buffers returns
 *   every list in ascending key order,
 *   ambient_occlusion_denoiser ("None" | "Edge-Avoiding A-Trous Wavelet Transform" (UTF-8 A-grave as in Denoiser.hpp:66; "EAW"
 *   is accepted too) | "SVGF" | "Spatial Hashing")                     (VulkanRayTracedAmbientOcclusion.cpp:683-696)
 *   eaw_denoiser_iterations (0..5, default 3), eaw_denoiser_color_weights / _position_weights / _normal_weights,
 *   eaw_denoiser_phi_color / _phi_position / _phi_normal, eaw_denoiser_use_shared_memory   (EAWDenoiser.cpp:400-432)
 *   svgf_denoiser_iterations (0..5, default 5), svgf_denoiser_allowed_z_dist (0.002), svgf_denoiser_allowed_normal_dist
 *   (0.02): build-owned keys for parameters the reference exposes in its GUI only (SVGF.hpp:70-72,115).  SVGF is
 *   temporal: every lv_render* call advances its history (one step per RTAO iteration), always over the whole viewport;
 *   lv_set_lines resets the global frame counter, a change of the denoiser or of the viewport size clears the history,
 *   "Spatial Hashing" (SpatialHashingDenoiser.cpp, SH_Denoise.glsl; the order-independent statement of linevis_amd/csrc/lv_sh.h): the
 *   AO of every RTAO iteration is accumulated in world space, in a hash map of multi-resolution cells keyed by position and normal,
 *   read back per hit and smoothed by three a-trous passes with fixed settings.  Like SVGF it takes the iteration's own AO image and
 *   the global frame number, and runs over the whole viewport after every RTAO iteration.  Build-owned keys for what the reference
 *   exposes in its GUI only: spatial_hashing_s_p (cell size in pixels, 0.1 ... 20, default 8), spatial_hashing_s_min_exp (smallest
 *   cell 10^exp, -20 ... -1, default -17), spatial_hashing_s_nd (normal coarseness, 1 ... 10, default 3), spatial_hashing_num_cells
 *   (>= 10, default 10000000; 16 B each, allocated while the denoiser is selected), spatial_hashing_atomics_mode ("Uint Quantized
 *   Atomic Add"; "Float Atomic Add", "Uint Spinning Atomic Add" and "No Atomics" are refused: a float sum or a racing write depends
 *   on the execution order).  The map survives camera and viewport changes; it is cleared when more than half of its cells are occupied, before a count
 *   could reach 2^28, by lv_set_lines / lv_set_trajectories, a changed line_width, s_p, s_min_exp, s_nd or num_cells, and by
 *   lv_spatial_hashing_reset.  A contribution that finds ten other keys in its probe window is dropped and counted (no eviction),
 *   band data (ribbons; the ray tracer's closest-hit paths: analytic geometry modes, or "Triangle Mesh" / rtao_geometry =
 *   triangle_tubes on the elliptic triangle tubes lv::LineDataFlow tessellates for such data; use_mlat over the same
 *   geometries; the PPLL gather over the analytic tubelets / capsules; the static prebaker: ray origins on the elliptic cross-
 *   section, traced against the elliptic triangle tubes passed to lv_set_tube_triangle_mesh, VulkanAmbientOcclusionBaker.glsl:200-257):
 *   use_ribbons (= USE_BANDS: the line points passed to
 *   lv_set_lines come from a data set with ribbon directions and ribbons are on, LineDataFlow.cpp:587-606,2423-2431),
 *   thick_bands, min_band_thickness (0.15, LineData.cpp:54), band_width (0.005, LineRenderer.cpp:442-449,
 *   DataSetList.hpp:47), use_analytic_elliptic_tubes (build-owned key for the ray tracer's "Elliptic Tubes" checkbox,
 *   VulkanRayTracer.cpp:198-201: the points then carry the ribbon normals of getLinePassTubeAabbRenderData(false, true)
 *   and every segment is a sphere-traced elliptic tubelet, EllipticTubeRayTracing.glsl).
 *   rotating helicity bands of flow lines (USE_ROTATING_HELICITY_BANDS, LineDataFlow.cpp:601-624,2432-2440; excludes
 *   use_ribbons): rotating_helicity_bands (the line points then carry lineRotation, LineDataFlow.cpp:2188-2197),
 *   separator_width (0.2), band_subdivisions (6), helicity_rotation_factor (1), use_uniform_twist_line_width (true;
 *   UNIFORM_HELICITY_BAND_WIDTH, "Triangle Mesh" geometry only: LineAttributesBarycentric.glsl:94-112). */
int lv_set_option(lv_ctx* ctx, const char* key, const char* value);

/* LineData::getRayTracingTubeAabbTopLevelAS (LineData.cpp:1057-1075) + getTubeAabbBottomLevelAS (:879-907):
 * builds the LBVH over segment AABBs min(p0,p1)-r .. max(p0,p1)+r (LineDataFlow.cpp:2230-2233) on the GPU.
 * Called implicitly by lv_render* when lines or line_width changed.  The tube mesh and its triangle LBVH are built along
 * with it only while the current options use them (RTAO on triangle tubes, the prebaker, geometry_mode "Triangle Mesh");
 * every other frame that needs them later builds them itself. */
int lv_build_accel(lv_ctx* ctx);

/* LineRenderer::render() (LineRenderer.hpp:112) for mode 11 (VulkanRayTracer::render, VulkanRayTracer.cpp:131-154:
 * depth range -> RTAO iterations -> colour pass) or mode 2 (PerPixelLinkedListLineRenderer::render,
 * PerPixelLinkedListLineRenderer.cpp:399-427: clear -> gather -> resolve) or mode 3 (MLABRenderer::render: the same
 * gather, then the fold and resolve of MLAB) or mode 6 (MBOITRenderer::render, MBOITRenderer.cpp:472-482: depth range -> the
 * same gather -> moments, reconstruction and blend) restricted to the pixel rectangle
 * [x0, x0+w) x [y0, y0+h) of the viewport.  out: w*h*4 bytes. */
int lv_render(lv_ctx* ctx, int rendering_mode, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint8_t* out_rgba8);
int lv_render_device(lv_ctx* ctx, int rendering_mode, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                     void* out_rgba8_device);

/* Same for a list of equally sized tiles (screen-tile sharding).  tiles_xy: 2 uint32 per tile
 * (pixel origin).  Output is tile-major: [num_tiles][tile_h][tile_w][4]; parts of a tile outside the viewport are
 * written as the background colour. */
int lv_render_tiles_device(lv_ctx* ctx, int rendering_mode, const uint32_t* tiles_xy, uint32_t num_tiles,
                           uint32_t tile_w, uint32_t tile_h, void* out_rgba8_device);

/* ---- several GPUs behind one handle (SURVEY.md 8b "Multi-GPU = one context per device", 8e; the reference is single-GPU:
 * sgl::AppSettings::getPrimaryDevice() everywhere, e.g. src/LineData/LineData.cpp:722) ----
 * lv_create_multi: one context per listed device, driven through the returned handle (= rank 0, the first device) by the calling
 * thread; every setter above is repeated on all ranks (full scene replica + LBVH per GPU), every lv_render* call deals the
 * requested pixels as screen tiles over the ranks (64 x 64 along a Morton order for a rectangle; the caller's tiles for
 * lv_render_tiles_device), renders them concurrently and assembles them on rank 0 with ONE gather of RGBA8 tiles:
 * transport "rccl" (default; ncclSend / ncclRecv group over xGMI, librccl resolved at run time; distinct devices) or "memcpy"
 * (hipMemcpyPeerAsync + events; no RCCL needed, the same device may appear several times).  The frame is byte-identical to the
 * single-device frame.  Output pointers of lv_render_device / lv_render_tiles_device live on the first device.  Read-backs
 * (lv_get_ao, lv_ppll_get_buffers, lv_get_kernel_times, ...) address rank 0; lv_get_stats sums the counters of all ranks.
 * lv_multi_rebalance: re-deals the tiles of the last frame by measured cost (RTAO hit pixels x samples per tile + base_cost_per_tile,
 * longest processing time first); synchronises all ranks, call it between frames (progressive accumulation: not while a
 * num_accumulated_frames > 1 sequence is running -- the history stays on the rank that rendered it).  A tile list that differs
 * from the previous call's (another rectangle, other tiles) starts from a fresh round-robin deal: the cost-weighted deal belongs to
 * the list it was measured on.  A rank that owns no tile of a frame (fewer tiles than ranks) renders the list's first tile for
 * itself, so that its temporal state (RTAO seed counter, SVGF history) stays in step with the other ranks'.
 * lv_multi_deal: tile -> rank of the last frame.  lv_tile_deal / lv_make_tiles: the deal and the tile order as pure host
 * functions (costs == NULL: round robin). */
lv_ctx* lv_create_multi(const int* device_ordinals, int num_devices, const char* transport, int* err);
int lv_multi_ranks(const lv_ctx* ctx);
/* lv_get_stats of ONE rank of a multi-device handle (its own counters, phase times and kernel timings, nothing summed): what a
 * scaling run needs to see which rank a frame waited for.  rank 0 = the handle's own device; a single-device context has rank 0 only. */
int lv_multi_rank_stats(lv_ctx* ctx, int rank, lv_stats* out);
int lv_multi_rebalance(lv_ctx* ctx, double base_cost_per_tile);
int lv_multi_deal(lv_ctx* ctx, uint32_t* out_owner, uint32_t capacity, uint32_t* out_count);
int lv_tile_deal(const double* costs, uint32_t num_tiles, uint32_t num_ranks, uint32_t* out_owner);
uint32_t lv_make_tiles(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t tile, uint32_t* out_xy, uint32_t capacity);

int lv_get_stats(lv_ctx* ctx, lv_stats* out);
/* Forget the per-kernel launch timings collected so far (start of a timed benchmark region). */
int lv_reset_timers(lv_ctx* ctx);
/* Individual launch durations (ms, oldest first) of kernel `kernel_id` (LV_KERNEL_*) since lv_reset_timers(), at most the
 * last 512: what a benchmark needs for a median / p95 (the reference's analogue: the per-phase GPU timers of
 * PerPixelLinkedListLineRenderer.cpp:411-420 / AutomaticPerformanceMeasurer).  Synchronises the stream. */
int lv_get_kernel_times(lv_ctx* ctx, int kernel_id, float* out_ms, uint32_t capacity, uint32_t* out_count);

/* Hit pixels (primary rays of the RTAO pass that hit geometry) per 64x64-pixel group of the last lv_render* call's tile
 * list, in tile-list order, `*out_groups_per_tile` consecutive entries per tile: a rank's per-tile AO cost (AO rays = hit
 * pixels x samples), which the tile sharding uses to re-deal tiles by cost (linevis_amd/tiling.py; SURVEY.md 8e asks for
 * load balance by tile dealing -- the reference itself is single-GPU).  LV_E_STATE unless the last call ran the RTAO pass. */
int lv_get_ao_tile_costs(lv_ctx* ctx, uint32_t* out_counts, uint32_t capacity, uint32_t* out_count, uint32_t* out_groups_per_tile);

/* Dispatch order of the tile kernels (option dispatch_order = cost, the default): the 64x64-pixel groups of the last
 * lv_render* call's tile list in the order their workgroups were started -- heaviest group of the frame before first (longest
 * processing time first; groups are numbered tile-major, `groups per tile` consecutive entries per tile) -- and what every
 * group cost in the last call (device clock ticks summed over its waves: the input of the next call's order).  No counterpart
 * in the reference (the Vulkan driver schedules its ray-generation workgroups); which workgroup renders which group never
 * shows in the image.  *out_count = 0 when the order is off or the launch has fewer than 2 / more than 8192 groups. */
int lv_get_dispatch_order(lv_ctx* ctx, uint32_t* out_order, uint32_t* out_cost, uint32_t capacity, uint32_t* out_count);

/* ---- streamline tracing: the producer of the line sets ----
 * StreamlineTracingGrid (src/LineData/Flow/StreamlineTracingGrid.cpp): regular grid of xs*ys*zs cells with spacing
 * (dx, dy, dz) and origin 0 (setGridExtent, :81-116), one vector field (3 floats per cell, x fastest: IDXV of
 * StreamlineTracingDefines.hpp:118) and any number of scalar fields sampled along the lines as attributes
 * (_pushTrajectoryAttributes, :1012-1047).  max |v| (addVectorField, :189-216) is reduced on the GPU. */
int lv_set_flow_grid(lv_ctx* ctx, const float* vector_field, uint32_t xs, uint32_t ys, uint32_t zs, float dx, float dy,
                     float dz, const float* const* scalar_fields, uint32_t num_scalar_fields);
/* StreamlineTracingSettings, StreamlineTracingDefines.hpp:144-177 (the fields _trace / traceStreamlines read). */
typedef struct lv_streamline_settings {
    uint32_t integration_method;    /* StreamlineIntegrationMethod :63-76: 0 explicit Euler, 1 implicit Euler, 2 Heun,
                                     * 3 midpoint, 4 RK4, 5 Runge-Kutta-Fehlberg (double precision, adaptive step) */
    uint32_t integration_direction; /* StreamlineIntegrationDirection :82-84: 0 forward, 1 backward, 2 both */
    float time_step_scale;          /* 1.0 */
    int32_t max_num_iterations;     /* 2000 */
    float termination_distance;     /* 1.0 (scaled by 1e-6 inside, :1199) */
    float minimum_length;           /* 0.7: shorter lines are dropped (:413-425) */
} lv_streamline_settings;
/* StreamlineTracingGrid::traceStreamlines (:344-426) for caller-supplied seed points (3 floats each): one GPU thread per
 * seed and direction integrates (_trace, :1193-1259), the host part reverses / merges / filters.  The result stays in the
 * context until the next call; fetch it with lv_get_streamlines. */
int lv_trace_streamlines(lv_ctx* ctx, const float* seed_points, uint32_t num_seeds, const lv_streamline_settings* settings,
                         uint64_t* out_num_lines, uint64_t* out_num_points);
/* positions: 3 floats per point; attributes: [num_scalar_fields][num_points]; line_offsets: num_lines + 1.  Any pointer
 * may be NULL. */
int lv_get_streamlines(lv_ctx* ctx, float* positions, float* attributes, uint32_t* line_offsets);

/* StreamlineMaxHelicityFirstSeeder + StreamlineTracingGrid::_traceStreamribbonsDecreasingHelicity (StreamlineSeeder.cpp:360-529,
 * StreamlineTracingGrid.cpp:546-860; Rees et al., "A stream ribbon seeding strategy", EuroVis 2017): the grid points (or, with a
 * subsampling factor, the centres of blocks of cells) are seeded in the order of falling helicity; a line ends where it enters a
 * cell within minimum_separation_distance of an earlier line's point, and a sample whose cell is taken is skipped.  The reference
 * traces these lines one after the other on the CPU; here batches of the next seeds are traced speculatively in parallel on the GPU
 * and committed in seeding order on the host, each line cut where an earlier line of its batch claimed the cell first -- the same
 * lines, point for point.  Built: all four termination_check_types (1 = grid-based, the reference's default; 0 / 2 / 3 = naive /
 * k-d tree / hashed grid: a line ends where it comes within minimum_separation_distance of a POINT of an earlier line -- the lines
 * are cut on the host by that exact predicate, the device tests against the points finished before the batch), all five loop_check_modes (the
 * per-line state of "All Points" / "Grid" / "Curvature" lives in the tracing thread; sgl's HashedGrid and CircularQueue are not
 * vendored: the sphere query is distance <= radius over the line's own points, the queue a FIFO of 32; acos of "Curvature" is the
 * build's fixed formula; getHasPointCloserThan of sgl's KdTree / HashedGrid: distance < r like the naive loop's glm::distance test);
 * not built: Runge-Kutta-Fehlberg (its step width carries over from line to line in the reference).  helicity_field: xs * ys * zs floats (computeHelicityFieldNormalized).
 * The result is fetched with lv_get_streamlines like lv_trace_streamlines'. */
typedef struct lv_helicity_seeding_settings {
    float minimum_separation_distance;   /* 0.08, StreamlineTracingDefines.hpp:158 */
    uint32_t termination_check_type;      /* TerminationCheckType :89-94: 0 naive, 1 grid-based (the default), 2 k-d tree-based, 3 hashed
                                           * grid-based.  0 / 2 / 3 are one predicate -- a point of a finished line closer than
                                           * minimum_separation_distance -- behind three searches in the reference, one here (a uniform
                                           * grid of the finished points in HBM); 0 does not filter the seeds (StreamlineSeeder.cpp:452) */
    uint32_t loop_check_mode;             /* LoopCheckMode :99-101: 0 none, 1 start point, 2 all points, 3 grid, 4 curvature */
    float termination_distance_self;      /* 1.0 (:156): start-point loop check within |box| / 100 times this */
    int32_t seeding_subsampling_factor;   /* 1 (:174) */
} lv_helicity_seeding_settings;
int lv_trace_streamlines_max_helicity_first(lv_ctx* ctx, const float* helicity_field, const lv_streamline_settings* settings,
                                            const lv_helicity_seeding_settings* seeding, uint64_t* out_num_lines,
                                            uint64_t* out_num_points);
/* Per line of the last result: the index of the seed point inside the merged line (0 for forward lines, the last point for
 * backward ones, behind the reversed backward part otherwise).  Streamribbons carry their ribbon direction outwards from the
 * seed in both parts (StreamlineTracingGrid::traceStreamribbons, StreamlineTracingGrid.cpp:428-530). */
int lv_get_streamline_seed_indices(lv_ctx* ctx, uint32_t* out_seed_index);

/* ---- inspection entry points used by the parity tests ---- */
/* Closest hit of arbitrary rays (IntersectionTube + driver closest-hit semantics, TubeRayTracing.glsl:452-494).
 * origins/dirs: 3 floats per ray; out_segment = 0xFFFFFFFF on miss; out_kind: 0 tube, 1 sphere p0, 2 sphere p1. */
int lv_trace_rays(lv_ctx* ctx, const float* origins, const float* dirs, float t_min, float t_max, uint32_t n,
                  float* out_t, uint32_t* out_segment, uint32_t* out_kind);
/* Same against the triangle tubes (the driver's triangle test is restated as Moeller-Trumbore without culling + "t inside
 * the triangle's own padded AABB interval").  out_triangle = 0xFFFFFFFF on miss, ties -> lowest triangle
 * index; out_uv (2 floats per ray, may be NULL) = barycentrics as rayQueryGetIntersectionBarycentricsEXT. */
int lv_trace_rays_triangles(lv_ctx* ctx, const float* origins, const float* dirs, float t_min, float t_max, uint32_t n,
                            float* out_t, uint32_t* out_triangle, float* out_uv);
/* Same against the simulation-mesh hull (lv_set_hull_mesh) with the hull's own pad (hull_ray_tracing above): the closest hull hit H of
 * csrc/lv_hull_rt.h, t inside [t_min, t_max].  Works whatever hull_ray_tracing and hull_opacity say; builds the hull's LBVH if no frame
 * has yet.  LV_E_STATE without a mesh. */
int lv_trace_rays_hull(lv_ctx* ctx, const float* origins, const float* dirs, float t_min, float t_max, uint32_t n,
                       float* out_t, uint32_t* out_triangle, float* out_uv);
/* The steps of every pixel's transparency loop in the last whole-viewport mode-11 frame rendered with rt_record_hits (lv_render, or a
 * tile list that covers the viewport without overlap; not with use_mlat): 9 uint32 per record {viewport pixel index y * W + x,
 * sampleIdx << 16 | hitIdx, primitive, bits of t, bits of payload.hitT, bits of the hit's straight colour r, g, b, a}; primitive = bit
 * 31 | hull triangle index for a hull hit, else original segment << 2 | kind (lv_trace_rays' kinds; original triangle << 2 in the
 * Triangle Mesh geometry mode).  A miss is not recorded; records arrive in no particular order.  *out_count is always the number the
 * frame produced; more than the rt_hits_capacity that frame ran with (raising the option afterwards does not help: render again), or
 * than max_records with out_records given, returns LV_E_CAPACITY.  out_records may be
 * NULL (query the count).  LV_E_STATE when the last frame recorded nothing. */
int lv_rt_get_hits(lv_ctx* ctx, uint32_t* out_records, uint64_t max_records, uint64_t* out_count);
/* LineRenderer::computeDepthRange (LineRenderer.cpp:410-431): min/max view depth of all line points. */
int lv_compute_depth_range(lv_ctx* ctx, float out_min_max[2]);
/* Full-viewport RTAO texture (.x channel of the RGBA32F accumulation image) after the last mode-11/2 render. */
int lv_get_ao(lv_ctx* ctx, float* out /* viewport_width * viewport_height */);
/* MLAT (use_mlat) parity instrument: the order in which every pixel's candidates were handed to insertNodeMlat in the
 * last mode-11 render (options collect_stats + mlat_record_trace).  4 uint32 per record {viewport pixel index y * W + x,
 * sequence number within the pixel, original segment index (triangle index in the Triangle Mesh mode), flag: 0 = inserted, 1 = dropped because an accepted hit had
 * already shortened the ray interval}; records arrive in no particular order.  The reference's own order is the driver's
 * BVH traversal order (undefined); a CPU replay of THIS order must reproduce the frame.  out_records may be NULL
 * (query the count). */
int lv_get_mlat_trace(lv_ctx* ctx, uint32_t* out_records, uint64_t max_records, uint64_t* out_count);
/* Parity instrument without a reference counterpart: the shading kernels evaluate normalize(v) = v * r(v . v), r(x) = the IEEE-correct
 * bits of 1.0f / sqrtf(min(max(x, 2^-60), 2^60)) (the CPU checker states the same rule), through a shortened instruction sequence.
 * Runs that sequence on ALL 2^32 float arguments on the device against the rule evaluated with the compiler's own division and square
 * root; out_mismatches = number of arguments whose results differ in any bit (NaN results count as equal to each other),
 * out_first_argument = the bits of one of them. */
int lv_selftest_rsqrt(lv_ctx* ctx, uint64_t* out_mismatches, uint32_t* out_first_argument);
/* Parity instrument without a reference counterpart: the traversal stack of the ray kernels (a window of LDS slots over a per-thread
 * column of a global slab, spilled and refilled in blocks) run on scripts.  One workgroup of 256 threads with the window and stride
 * of the RTAO sample kernel (LV_STACK_INST_AO) or of the tile kernels (LV_STACK_INST_TILE); thread t executes ops[t][0 .. ops_per_thread),
 * four words per operation: {code | keep flags, c3, c2, c1}.  LV_STACK_OP_PUSH3 is a node step's push of c3, c2, c1 in that order, each
 * kept only if its flag (bit 8, 9, 10) is set; LV_STACK_OP_POP appends the popped word (LV_INVALID: the stack is empty; only
 * LV_STACK_OP_CLEAR may follow) to out_words[t][...]; LV_STACK_OP_CLEAR drops every entry; LV_STACK_OP_END does nothing.
 * out_counts[t] = {words popped, blocks spilled, blocks refilled}.  The slab is sized by the routine that sizes it for a launch, for a
 * tree of wide_levels levels (at most 3 * wide_levels + 2 entries): a script that goes deeper, or pushes a word that is no node or
 * leaf reference (index < 2^26), is refused with LV_E_INVALID before anything runs.
 * out_info (may be NULL) = {entries of the LDS window, entries per spilled block, slab entries per thread for wide_levels, bytes of
 * slab the context's launches had reserved before this call, levels of the context's segment tree, of its triangle tree};
 * ops_per_thread == 0 only fills out_info.  tests/test_gpu_stack_spill.py compares with a plain list. */
#define LV_STACK_INST_AO 0
#define LV_STACK_INST_TILE 1
#define LV_STACK_OP_END 0
#define LV_STACK_OP_PUSH3 1
#define LV_STACK_OP_POP 2
#define LV_STACK_OP_CLEAR 3
int lv_selftest_stack(lv_ctx* ctx, uint32_t instantiation, uint32_t wide_levels, const uint32_t* ops /* 256 x ops_per_thread x 4 */,
                      uint32_t ops_per_thread, uint32_t* out_words /* 256 x ops_per_thread */, uint32_t* out_counts /* 256 x 3 */,
                      uint64_t* out_info /* 6 */);
/* Parity instrument without a reference counterpart: one of the build-owned scalar definitions evaluated on the
 * device for n arguments, by the same inline functions the render kernels call.  in_words / out_words are host arrays of bit
 * patterns (a float travels as its 32 bits), element-major: n x arity words in, n x results words out.  Uploads, launches one
 * kernel on the context's stream, synchronises and downloads.  LV_E_INVALID for a null pointer or an unknown id; n == 0 succeeds
 * without a launch.  tests/test_gpu_math.py compares the words with the CPU checker's, bit for bit (two NaNs count as equal).
 *
 * id (arguments -> results) and the domain on which host and device are bound to agree; tests/math_args.py holds each excluded
 * set as a named predicate:
 *   LV_FN_SINCOS2PI (xi -> sin, cos)        all floats except finite |xi| >= 2^29 (math_args.sincos2pi_outside_domain): the quadrant
 *                                           int(floor(4 xi)) does not fit an int there; callers pass [0, 1] or lv_sincos_rad's fraction
 *   LV_FN_SINCOS_RAD (a -> sin, cos)        all floats (non-finite a: the angle 0)
 *   LV_FN_ATAN2_DET (y, x -> angle)         all floats
 *   LV_FN_POW_DET (x, y -> x^y)             all floats (x < 0, x NaN, x denormal: the x == 0 rule)
 *   LV_FN_LOG2_DET (x -> log2 x)            all floats, bit for bit; a logarithm only for normal x > 0
 *   LV_FN_EXP2_DET (p -> 2^p)               all floats
 *   LV_FN_RSQRT_SHADE (x -> r(x))           all floats (lv_selftest_rsqrt)
 *   LV_FN_TEA (val0, val1 -> word), LV_FN_RND (seed -> next seed, value in [0, 1))   all words
 *   LV_FN_TRANSFER_FUNCTION (attribute -> rgba)   all floats and any range, attr_min == attr_max and infinite bounds included: the
 *                                           position is clamped to [0, 1] before anything is converted, a NaN position counts as 0
 *   LV_FN_TWIST_SAMPLE (u, dudx, dudy, use_grad != 0 -> rgba)   all floats: the texel coordinate goes through a saturating conversion
 *                                           (NaN -> 0, beyond the int range -> INT_MIN / INT_MAX) before it is wrapped
 *   LV_FN_PACK_UNORM4X8 (r, g, b, a -> word), LV_FN_UNPACK_UNORM4X8 (word -> r, g, b, a), LV_FN_STORE_RGBA8 (r, g, b, a -> the
 *                                           frame's pixel word, no accumulation)   all floats / words (a NaN channel stores 0)
 *   LV_FN_MBOIT_FIXED (term -> low, high word of the int64), LV_FN_MBOIT_UNFIXED (low, high -> float), LV_FN_MBOIT_SATURATE   all
 *   LV_FN_RSQRT_FAST, LV_FN_DIV_FAST (a, b), LV_FN_POW_FAST (x, y)   shading_numerics = fast: no host twin, accuracy bars in DESIGN.md §4
 * The transfer function and the twist sampler read the context's table, attribute range, texture and filtering mode (LV_E_STATE
 * while none is set); no line data is needed. */
#define LV_FN_SINCOS2PI 1
#define LV_FN_SINCOS_RAD 2
#define LV_FN_ATAN2_DET 3
#define LV_FN_POW_DET 4
#define LV_FN_LOG2_DET 5
#define LV_FN_EXP2_DET 6
#define LV_FN_RSQRT_SHADE 7
#define LV_FN_TEA 8
#define LV_FN_RND 9
#define LV_FN_TRANSFER_FUNCTION 10
#define LV_FN_TWIST_SAMPLE 11
#define LV_FN_PACK_UNORM4X8 12
#define LV_FN_UNPACK_UNORM4X8 13
#define LV_FN_STORE_RGBA8 14
#define LV_FN_MBOIT_FIXED 15
#define LV_FN_MBOIT_UNFIXED 16
#define LV_FN_MBOIT_SATURATE 17
#define LV_FN_RSQRT_FAST 18
#define LV_FN_DIV_FAST 19
#define LV_FN_POW_FAST 20
int lv_selftest_eval(lv_ctx* ctx, uint32_t function_id, const uint32_t* in_words, uint64_t n, uint32_t* out_words);
/* PPLL buffers after the last mode-2 render: nodes = 3 uint32 {rgba8, depth bits, next} per node slot (slots are handed
 * out to waves in chunks, so unreferenced slots may lie between the stored fragments), start_offset = padded_w * padded_h
 * heads (0xFFFFFFFF = empty), frag_counter = number of fragments generated.  Either pointer may be NULL. */
int lv_ppll_get_buffers(lv_ctx* ctx, uint32_t* out_nodes, uint64_t max_nodes, uint32_t* out_start_offset,
                        uint64_t max_pixels, uint32_t* out_frag_counter);
/* Resolve caller-supplied PPLL buffers (LinkedListResolve.glsl:57-105) with the current camera/options. */
int lv_ppll_resolve_buffers(lv_ctx* ctx, const uint32_t* nodes, uint64_t num_nodes, const uint32_t* start_offset,
                            uint64_t num_pixels, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                            uint8_t* out_rgba8);
/* Test entry point of mode 3's fold (MLABGather.glsl:38-60 in primitive order + MLABResolve.glsl:51-77 + the blend over the
 * background), the counterpart of lv_ppll_resolve_buffers.  entries = 3 uint32 per fragment {packUnorm4x8(rgb * a, 1 - a), window
 * depth (float bits), primitive key}; pixel p = y * w + x of the w x h rectangle owns entries [offsets[p], offsets[p + 1])
 * (offsets: w * h + 1 values from 0 to num_entries) in any order -- they are folded in ascending key order.  Keys are unique within
 * a pixel and not 0xFFFFFFFF; at most 65535 entries per pixel.  K = mlab_num_layers. */
int lv_mlab_resolve_buffers(lv_ctx* ctx, const uint32_t* entries, uint64_t num_entries, const uint64_t* offsets, uint32_t w,
                            uint32_t h, uint8_t* out_rgba8);
/* Test entry point of mode 6's two sweeps (MBOITPass1.glsl + MomentOIT.glsl generateMoments, MBOITPass2.glsl + resolveMoments,
 * MBOITBlend.glsl and the blend over the background).  entries = 5 uint32 per fragment: the float bits of {r, g, b, a, view depth}
 * (depth bits 0xFFFFFFFF are reserved); pixel p = y * w + x owns entries [offsets[p], offsets[p + 1]) in any order, at most 65534
 * per pixel.  N = mboit_num_moments; overestimation and bias from the options.  out_moments (may be NULL): w * h * (1 + N)
 * floats, b_0 then the normalised b_1 ... b_N of each pixel, zeros where b_0 is under the threshold. */
int lv_mboit_resolve_buffers(lv_ctx* ctx, const uint32_t* entries, uint64_t num_entries, const uint64_t* offsets, uint32_t w,
                             uint32_t h, float log_depth_min, float log_depth_max, float* out_moments, uint8_t* out_rgba8);
/* The *_get_* calls below (lv_mboit_get_moments, lv_atomic_loop_get_num_layers / _get_buffers, lv_wboit_get_buffers,
 * lv_depth_complexity_get_buffers / _get_stats, lv_depth_peeling_get_buffers) read what the last frame left on the device.  The
 * context keeps ONE record of that frame: lv_render of any mode replaces it, and every *_resolve_buffers test entry point of modes
 * 3, 6, 8, 9 and 10 clears it (they overwrite the per-pixel counts and the counters), whichever mode it belongs to.  After such a
 * call every *_get_* call returns LV_E_STATE until the next frame of its mode.
 *
 * The moments of the last frame when that was a mode-6 frame with mboit_fragment_storage = streamed over the whole viewport:
 * width * height * (1 + N) floats, row-major, in the layout of out_moments above (b_0, then the normalised b_1 ... b_N, zeros
 * where b_0 is under the threshold).  LV_E_STATE when the last frame was anything else (pooled storage, another mode, a tile list
 * that does not cover the viewport, a multi-device handle); LV_E_INVALID for a null pointer or capacity_floats below that size;
 * LV_E_CAPACITY when a pixel of that frame holds more than 131071 kept fragments.  Synchronises the context's stream. */
int lv_mboit_get_moments(lv_ctx* ctx, float* out, uint64_t capacity_floats);
/* K of the last frame when that was a mode-10 frame, else LV_E_STATE: the layer count lv_atomic_loop_get_buffers writes per pixel.  It
 * is the frame's, not the option's current value -- size out_slots by it when the option may have changed since the frame. */
int lv_atomic_loop_get_num_layers(lv_ctx* ctx, uint32_t* out_num_layers);
/* The slots and tail sums of the last frame when that was a mode-10 frame over the whole viewport, row-major: out_slots = width *
 * height * K keys (K = that frame's atomic_loop_num_layers, see lv_atomic_loop_get_num_layers; ascending, then 0xFFFFFFFFFFFFFFFF), out_tail = width * height * 5 sums
 * {SA, SR, SG, SB, SL}.  LV_E_STATE when the last frame was anything else (another mode, a tile list that does not cover the
 * viewport, a multi-device handle); LV_E_INVALID for a null pointer or capacity_pixels below width * height; LV_E_CAPACITY when a
 * pixel of that frame holds more than 131071 kept fragments.  Synchronises the context's stream. */
int lv_atomic_loop_get_buffers(lv_ctx* ctx, uint64_t* out_slots, uint64_t* out_tail, uint64_t capacity_pixels);
/* Test entry point of mode 10's insert and resolve: pixel p = y * w + x of the w x h rectangle owns keys [offsets[p], offsets[p + 1])
 * (offsets: w * h + 1 values from 0 to num_keys), at most 131071 per pixel, none 0xFFFFFFFFFFFFFFFF; equal keys are allowed.  The
 * keys are inserted on the device, one lane per key with all lanes racing, then resolved over the background.  K =
 * atomic_loop_num_layers.  out_slots (w * h * K) and out_tail (w * h * 5) may be NULL. */
int lv_atomic_loop_resolve_buffers(lv_ctx* ctx, const uint64_t* keys, uint64_t num_keys, const uint64_t* offsets, uint32_t w,
                                   uint32_t h, uint8_t* out_rgba8, uint64_t* out_slots, uint64_t* out_tail);
/* The sums and counts of the last frame when that was a mode-8 frame over the whole viewport, row-major: out_sums = width * height *
 * 5 sums {SR, SG, SB, SA, SL} (the 2^-36 fixed point), out_counts = width * height kept-fragment counts.  LV_E_STATE when the last
 * frame was anything else (another mode, a tile list that does not cover the viewport, a multi-device handle); LV_E_INVALID for a
 * null pointer or capacity_pixels below width * height; LV_E_CAPACITY when a pixel of that frame holds more than 131071 kept
 * fragments.  Synchronises the context's stream. */
int lv_wboit_get_buffers(lv_ctx* ctx, int64_t* out_sums, uint32_t* out_counts, uint64_t capacity_pixels);
/* Test entry point of mode 8's accumulation and resolve: pixel p = y * w + x of the w x h rectangle owns entries [offsets[p],
 * offsets[p + 1]) (offsets: w * h + 1 values from 0 to num_entries); an entry is 5 float words {r, g, b, alpha, window depth}.  The
 * fragments are added on the device, one lane per fragment with all lanes racing, under wboit_depth_weight, then resolved over the
 * background.  At most 131071 entries per pixel: more returns LV_E_CAPACITY (the resolve's flag).  out_sums (w * h * 5) may be NULL. */
int lv_wboit_resolve_buffers(lv_ctx* ctx, const uint32_t* entries, uint64_t num_entries, const uint64_t* offsets, uint32_t w, uint32_t h,
                             uint8_t* out_rgba8, int64_t* out_sums);
/* The kept-fragment counts of the last frame when that was a mode-5 frame over the whole viewport, row-major (width * height).
 * LV_E_STATE when the last frame was anything else (another mode, a tile list that does not cover the viewport, a multi-device handle);
 * LV_E_INVALID for a null pointer or capacity_pixels below width * height.  Synchronises the context's stream. */
int lv_depth_complexity_get_buffers(lv_ctx* ctx, uint32_t* out_counts, uint64_t capacity_pixels);
/* What the reference's performance measurer records per frame (pushDepthComplexityFrame): the sum of the counts, the pixels with at
 * least one fragment, the largest and the smallest count, and width * height.  (The reference reports used_locations = 1 for a frame
 * without fragments to avoid a division; here 0 stays 0.) */
typedef struct lv_depth_complexity_stats {
    uint64_t total;
    uint64_t used_locations;
    uint64_t max;
    uint64_t min;
    uint64_t buffer_size;
} lv_depth_complexity_stats;
/* The statistics of the last frame under the conditions of lv_depth_complexity_get_buffers, reduced on the device. */
int lv_depth_complexity_get_stats(lv_ctx* ctx, lv_depth_complexity_stats* out);
/* The accumulators {r, g, b, a} (float32, premultiplied, before the blit), the numbers of peeled layers and the kept-fragment counts of
 * the last frame when that was a mode-9 frame over the whole viewport, row-major.  Errors as lv_depth_complexity_get_buffers. */
int lv_depth_peeling_get_buffers(lv_ctx* ctx, float* out_accum_rgba, uint32_t* out_layers, uint32_t* out_counts, uint64_t capacity_pixels);
/* Test entry point of mode 9's passes and blit: pixel p = y * w + x of the w x h rectangle owns entries [offsets[p], offsets[p + 1])
 * (offsets: w * h + 1 values from 0 to num_entries); an entry is 6 words {r, g, b, alpha, window depth (float32), primitive key
 * (uint32)}.  min(longest run, depth_peeling_max_layers) passes with one lane per entry, all lanes racing for the pixel's slot.
 * Precondition: the keys of a pixel's entries are distinct.  out_accum_rgba (w * h * 4) and out_layers (w * h) may be NULL. */
int lv_depth_peeling_resolve_buffers(lv_ctx* ctx, const uint32_t* entries, uint64_t num_entries, const uint64_t* offsets, uint32_t w,
                                     uint32_t h, uint8_t* out_rgba8, float* out_accum_rgba, uint32_t* out_layers);
/* The visibility buffer of the last frame when that was a mode-1 frame over the whole viewport, row-major: the primitive index
 * (0xFFFFFFFF: none) and the depth (1.0: none) of every pixel -- which triangle, hence which line, lies under a pixel, and the scene
 * depth.  Either array may be NULL.  LV_E_STATE if the last frame was not such a frame or the viewport changed since, LV_E_INVALID
 * if max_pixels < width * height. */
int lv_deferred_get_buffers(lv_ctx* ctx, uint32_t* primitive_index, float* depth, uint64_t max_pixels);
/* Test entry point of mode 1's shading pass: the caller's visibility buffer of w x h pixels, row-major (pixel p = y * w + x), shaded
 * into out (w * h RGBA8 words) with w x h as the viewport size, under the context's camera, options, transfer function and tube
 * triangle mesh.  LV_E_INVALID for a null array, an empty rectangle or a primitive index that is neither 0xFFFFFFFF nor below the
 * mesh's triangle count, and -- with the screen-space RTAO on -- a w x h other than the last RTAO image's; LV_E_STATE without camera,
 * transfer function or mesh, and with depth cues before the first frame.  The mesh is brought up to date first (the index check needs
 * its triangle count); nothing else of the context is touched before the checks pass, and a refused call leaves the last frame's
 * lv_deferred_get_buffers as it was. */
int lv_deferred_shade_buffers(lv_ctx* ctx, const uint32_t* primitive_index, const float* depth, uint32_t w, uint32_t h, uint32_t* out);
/* The simulation-mesh hull (LineData::simulationMeshOutline*, BinLinesLoader.cpp:107-121; LineRenderer::renderHull): an indexed
 * triangle mesh with three floats per vertex for the positions and for the normals, both required; the normals are used as given
 * (not renormalised).  Copied to HBM as 32-byte lv_hull_vertex records (8 * num_vertices + 3 * num_triangles words); every rank of
 * an lv_create_multi handle gets a replica.  num_triangles == 0 removes the mesh.  LV_E_INVALID, with the previous mesh left in
 * force, for a null array, an index >= num_vertices or a non-finite position or normal.  The mesh does not belong to the lines: it
 * stays until it is replaced or removed.  What draws it: hull_opacity above. */
int lv_set_hull_mesh(lv_ctx* ctx, const uint32_t* triangle_indices, uint32_t num_triangles, const float* positions, const float* normals,
                     uint32_t num_vertices);
/* The current hull mesh read back.  Any output pointer may be NULL (query the counts); LV_E_CAPACITY if a given array is too small. */
int lv_get_hull_mesh(lv_ctx* ctx, uint32_t* out_triangle_indices, uint32_t max_triangles, float* out_positions, float* out_normals,
                     uint32_t max_vertices, uint32_t* out_num_triangles, uint32_t* out_num_vertices);
/* Every kept hull fragment of the whole viewport under the current camera and options, unordered -- the hull's picking query and the
 * inspection entry point of its fragment stage: pixel = y * width + x, the triangle's index, the window depth, the straight float32
 * colour (4 floats per fragment).  No alpha discard: that belongs to a mode.  It does not ask whether a hull would be drawn
 * (hull_opacity is used as it stands).  *out_count is always the number of fragments; a smaller capacity returns LV_E_CAPACITY and
 * writes nothing else.  Any output array may be NULL.  LV_E_STATE without a hull mesh, camera or lines.  Touches nothing a *_get_*
 * call of the last frame reads. */
int lv_hull_get_fragments(lv_ctx* ctx, uint32_t* pixel, uint32_t* triangle, float* depth, float* rgba, uint64_t capacity,
                          uint64_t* out_count);
/* Every kept line-quad fragment of the last frame, when that was a mode-5, mode-8 or mode-10 frame over the WHOLE viewport (lv_render,
 * lv_render_device; not a tile list: such a frame fills the AO image for its tiles only) drawn with line_primitive_mode = "Quads
 * (Programmable Pull)": unordered, evaluated again on the line data, the AO image and the depth range the frame left in the context --
 * the inspection entry point of the quads' fragment stage, as lv_hull_get_fragments is the hull's.  pixel = y * width + x; segment: the
 * index of the segment in the caller's order; triangle: 0 = (2a, 2b, 2b + 1), 1 = (2a, 2b + 1, 2a + 1); the window depth; the straight
 * float32 colour (4 floats per fragment).  No alpha discard: that belongs to a mode.  *out_count is always the number of fragments; a
 * smaller capacity returns LV_E_CAPACITY and writes nothing else.  Any output array may be NULL.  LV_E_STATE when the last frame was no
 * such frame (a tube frame, a tile list, another mode, a refused call), and when what the pass reads is no longer the frame's: after
 * lv_set_lines / lv_set_trajectories[_with_bands], a changed line_width, a viewport of another size (lv_set_camera), or a change of
 * whether the lighting reads the AO image (ambient_occlusion_mode / _strength) -- render the frame again.  A camera pose, colour or
 * strength changed since the frame changes the answer only: call it before changing them.  Touches nothing a *_get_* call of the last
 * frame reads. */
int lv_line_quads_get_fragments(lv_ctx* ctx, uint64_t capacity, uint32_t* pixel, uint32_t* segment, uint32_t* triangle, float* depth,
                                float* rgba, uint64_t* out_count);
/* Test entry point of the SVGF denoiser: one SVGFDenoiser::denoise() (SVGF.glsl Compute-Reproject, Compute-Filter-Moments,
 * svgf_denoiser_iterations x Compute-ATrous, the history copies of SVGF.cpp) on caller-supplied images of w x h pixels (1 ... 16384
 * each), row-major.  Inputs: noisy = 1 float per pixel (the raw AO), normal_depth = 4 floats {world normal xyz, depth}, flow_fwidth =
 * 4 floats {flow x, flow y, depth fwidth, unused}.  The three history images are read and overwritten with this call's: color_history
 * = 1 float (colour after the first a-trous pass, or the filtered colour with 0 iterations), moments_history = 4 floats {m1, m2, history
 * length, 0}, normal_depth_history = 4 floats.  out = 1 float per pixel, the denoised image.  The thresholds come from the options
 * svgf_denoiser_allowed_z_dist / svgf_denoiser_allowed_normal_dist.  The renderer's own SVGF history is not touched.
 * Where SVGF.glsl leaves a result open, the rules are: texel fetches outside the image return 0; the moments filter reads the image
 * the reprojection pass wrote; `out` parameters the callee did not write keep 0 (moments) or the colour history at the pixel itself
 * (colour; it then enters with weight 0); max / min return the other operand of a NaN; pow(x, 128) is seven squarings; a reprojected
 * position ((0.5 + pixel) - flow or (0.01 + pixel) - flow) that is not finite or outside the int range fails
 * load_moments_and_history_length and is never converted to int; a non-finite depth fwidth drops the depth term of compute_weight.
 * LV_E_INVALID for a null pointer or an extent outside the range. */
int lv_svgf_denoise_buffers(lv_ctx* ctx, uint32_t w, uint32_t h, const float* noisy, const float* normal_depth,
                            const float* flow_fwidth, float* color_history, float* moments_history, float* normal_depth_history,
                            float* out);
/* Test entry point of the spatial-hashing denoiser: one Spatial_Hashing_Denoiser::denoise() (SH_Denoise.glsl Compute-Write and
 * Compute-Read as stated in linevis_amd/csrc/lv_sh.h, then three EAWDenoise.Compute passes with useColorWeights = false, phiPosition =
 * 0.3e-6, phiNormal = 0.1) on caller-supplied images of w x h pixels (1 ... 16384 each, fewer than 2^28 pixels), row-major.  Inputs:
 * noisy = 1 float per pixel (the iteration's AO; clamped to [0, 1], NaN counts as 0), normal_world = 4 floats {world normal xyz,
 * w}, position_world = 4 floats {world position xyz, w} (a pixel whose normal is (0, 0, 0) is a miss; finite values; all four
 * components enter the a-trous distances), cam_pos = 3 floats.  Outputs, 1 float per pixel: out_read (may be NULL) = the read pass'
 * image before the a-trous passes, 0 where nothing was read; out = the denoised image.  Cell sizes and the map size come from the
 * spatial_hashing_* options.  The call accumulates into a map of its own (map 1) that persists across calls; the renderer's map (map
 * 0) is not touched.  LV_E_INVALID for a null pointer or an extent outside the range. */
int lv_spatial_hashing_denoise_buffers(lv_ctx* ctx, uint32_t w, uint32_t h, const float* noisy, const float* normal_world,
                                       const float* position_world, const float* cam_pos, float* out_read, float* out);
/* Empties map `which` (0 = the renderer's, 1 = lv_spatial_hashing_denoise_buffers') and zeroes its statistics. */
int lv_spatial_hashing_reset(lv_ctx* ctx, int which);
/* The occupied cells of map `which`, in no particular order: keys[i] = (checksum << 32) | hash, accumulators[i] = (sum << 28) | count
 * with sum = the sum of floor(100 * occlusion + 0.5) and count = the number of contributions.  *count is always the number of
 * occupied cells; a smaller capacity returns LV_E_CAPACITY and writes nothing else.  Both arrays NULL: only the count. */
int lv_spatial_hashing_get_cells(lv_ctx* ctx, int which, uint64_t* keys, uint64_t* accumulators, uint64_t capacity, uint64_t* count);
/* out[0 .. 3] = {occupied, stored, dropped, clears} of map `which`: cells in use, contributions stored in and dropped from the map
 * since its last clear (stored + dropped = 4 x the hits written since then; the sum of all counts = stored), clears since the last
 * reset (lv_spatial_hashing_reset, a new spatial_hashing_num_cells). */
int lv_spatial_hashing_get_stats(lv_ctx* ctx, int which, uint64_t out[4]);
/* LBVH export for structural tests: compressed 4-wide nodes of 16 uint32/float words (64 B) each -- words 0-2 grid
 * origin xyz, words 3-5 grid scale xyz (floats), words 6-8 qmin x/y/z and words 9-11 qmax x/y/z (byte k = child slot
 * k; decoded plane = origin + q * scale), words 12-15 child references (bit 31 = leaf, 0xFFFFFFFF = empty slot);
 * leaf order = Morton order; see DESIGN.md. */
int lv_get_accel(lv_ctx* ctx, void* out_nodes, uint64_t max_nodes, uint32_t* out_leaf_segment, uint64_t max_leaves);

#ifdef __cplusplus
}
#endif
#endif /* LINEVIS_HIP_H */
