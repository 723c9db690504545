// lv_internal.h -- host-side context of the C-ABI library (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "lv_device.h"

struct LvDeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
};

// Temporal state of the SVGF denoiser (lv_svgf.hip): SVGF_Texture_Pack, SVGF.hpp
struct LvSvgfState {
    LvDeviceBuffer normalDepth, normalDepthHistory;   // float4 {world normal, depth}: this frame / previous frame
    LvDeviceBuffer flowFwidth;                        // float4 {flow.xy, depth fwidth, 0}
    LvDeviceBuffer moments, momentsHistory;           // float4 {m1, m2, history length, 0}
    LvDeviceBuffer colorHistory;                      // float: colour after the first a-trous pass of the previous frame
    LvDeviceBuffer tempAccum, tempAccumFiltered;      // float2 {colour, variance}: reprojection output, after the moments filter
    LvDeviceBuffer ping, pong;                        // float2: a-trous passes
    LvDeviceBuffer result;                            // float: the denoised AO image
    uint32_t width = 0, height = 0;
    bool historyValid = false;                        // false: clear the history images before the next frame
};

// Host-side state of a hash map of the spatial-hashing denoiser (lv_sh.hip; semantics in lv_sh.h).  The map itself -- numCells x 16 B
// {key word, accumulator}, vk_hash_map_buffer of SpatialHashingDenoiser.cpp:62-77 -- and its LvShCounters are device buffers of the context
struct LvShState {
    uint32_t numCells = 0;                            // cells of the allocated map; 0: none
    bool clearPending = false;                        // the next denoise starts with a forced clear (lines / line width / keying options changed)
    uint64_t pixelsSinceClear = 0;                    // bound on every cell's count since the last host-known clear (< 2^28)
    float sp = 0.0f, sNd = 0.0f;                      // the options the cells were keyed with
    int sMinExp = 0;
};

// Settings with the reference's defaults (file:line next to each value).
struct LvOptions {
    float lineWidth = 0.002f;                 // src/Loaders/DataSetList.hpp:46
    float depthCueStrength = 0.0f;            // reference default 0.8 (LineRenderer.hpp:220-221); off until set
    bool useAmbientOcclusion = false;         // ambient_occlusion_mode == "RTAO (Screen Space)" && strength > 0
    bool aoBakerIsRtao = false;
    float aoStrength = 0.0f;                  // LineRenderer.hpp (0 = off)
    float aoGamma = 1.0f;
    uint32_t aoIterations = 64;               // VulkanRayTracedAmbientOcclusion.hpp:108
    uint32_t aoSamplesPerFrame = 4;           // VulkanRayTracedAmbientOcclusion.hpp:150
    float aoRadius = 0.1f;                    // :151
    bool aoUseDistance = true;                // :152
    uint32_t triLeafSize = 2;                 // triangle_leaf_size: consecutive triangles per leaf of the triangle LBVH (1 ... 8)
    bool triLeafPairs = true;                 // triangle_leaf_records = pairs (64-B records of four vertices where every pair of triangles shares two, lv_bvh.hip) | triangles (48-B records)
    uint32_t treeletLeaves = 512;             // treelet_leaves: largest subtree the fast_trace build rebuilds (3 ... 4096)
    uint32_t treeletLaneLeaves = 6;           // treelet_lane_leaves: ranges of a treelet up to this size are built one lane per range (0 = the wave splits everything; 2 ... 64; measured: 0 4.5 ms, 4 3.8, 6 3.7, 8 3.9, 16 5.5 for the 1 M segments of config 3)
    uint32_t treeletGroupLeaves = 16;         // treelet_group_leaves: 0 | 8 | 16 -- ranges of <= 8 leaves are built by groups of 8 lanes, with 16 also those of 9 ... 16 leaves by groups of 16 (overrides treelet_lane_leaves; 1 M segments: 0 4.4 ms, 8 2.6, 16 2.4)
    uint32_t timerMask = 0xFFFFFFFFu;         // kernel_timers: bit LV_KERNEL_* = that kernel's launches are bracketed by HIP events, bit 31 = the frame's phase marks.
                                              // An event record costs the stream 2 - 4 us (a barrier packet): 12 of them are 6 % of a config-4 frame, 13 % of a config-2 frame
    bool collapseTop = true;                  // accel_collapse_top: the levels of the wide tree with <= 1024 nodes in one launch (k_collapse_top)
    bool treeletPlaneScan = true;             // treelet_plane_eval = scan (DPP prefix / suffix scans over the bins) | loop (round-3 form)
    bool accelFastTrace = true;               // accel_build = fast_trace (LBVH + SAH treelets, the reference's PREFER_FAST_TRACE) | fast_build (LBVH)
    bool accelPartitionSah = true;            // accel_partition = sah (fast_trace only: a binned-SAH partition chooses the leaf sets of the treelets, k_part_* in lv_bvh.hip) | morton (Morton order does)
    uint32_t accelPartitionMinLeaves = 65536; // accel_partition_min_leaves: builds of fewer leaves keep the Morton order under accel_partition = sah too (the partition's
                                              // levels cost two launches and a host round trip each whatever the size; its gain is measured on 1 M and 6 M leaves)
    bool fastShading = false;                 // shading_numerics = fast: approximate hardware rsq / rcp / log2 / exp2 in colour-only arithmetic (lv_device.h)
    int overlapPrimaryPasses = 2;             // overlap_primary_passes: 0 = false, 1 = true, 2 = auto -- the colour pass' hit traces in one launch with the RTAO primaries (k_primary_pair)
    bool dispatchByCost = true;               // dispatch_order = cost | as_numbered (tile kernels: heaviest 64x64 group of the last frame first)
    bool aoJitterPrimary = true;              // :153
    bool traceRaysHardwareInv = false;        // traversal_reciprocal = ieee (default) | hardware: lv_trace_rays / lv_trace_rays_triangles descend with lv_traversal_inv, the reciprocals of k_ao_rays (inspection of that path with arbitrary rays)
    bool aoPixelGeneration = true;            // ao_ray_generation = per_pixel (default: k_ao_rays sets up a batch of 64 AO rays per pixel when spp is a multiple of 64) | per_ray (the general path, forced)
    uint32_t numSamplesPerFrame = 1;          // VulkanRayTracer.hpp:137 has 2 (interactive); offline default 1
    uint32_t numAccumulatedFrames = 1;        // :142 (32 interactive); > 1: the caller renders frame_number = 0, 1, ...
    uint32_t frameNumber = 0;                 // accumulatedFramesCounter, VulkanRayTracer.cpp:141
    bool useDeterministicSampling = false;
    uint32_t maxDepthComplexity = 1024;       // VulkanRayTracer.hpp:139
    bool useCappedTubes = true;               // LineData.hpp:377-379
    bool useHalos = true;
    uint32_t tubeNumSubdivisions = 6;         // LineData.cpp:52
    uint32_t ppllSortingMode = 0;             // sorting_mode: index into SORTING_MODE_NAMES (PPLL.hpp:32-35), PerPixelLinkedListLineRenderer.hpp:113
    uint32_t ppllMaxNumFrags = 0;             // 0 = auto: 100 (<=1M segments) / 380, PerPixelLinkedListLineRenderer.hpp:45-49
    uint32_t ppllExpectedAvgDepthComplexity = 0; // 0 = auto: 20 / 120
    uint32_t ppllTileW = 2, ppllTileH = 8;    // LineRenderer.cpp:739-740
    bool collectStats = false;
    bool aoPrebaked = false;                  // ambient_occlusion_mode == "RTAO (Prebaker)"
    uint32_t bakeIterations = 128;            // VulkanAmbientOcclusionBaker.hpp:108
    uint32_t bakeNumTubeSubdivisions = 8;     // :165
    uint32_t bakeSamplesPerFrame = 4;         // :166 (radius / distance-based share the RTAO keys; same defaults :167-168)
    bool rtLss = false;                       // geometry_mode "Linear Swept Spheres" (VulkanRayTracer.hpp:56-63)
    bool rtTriangleMesh = false;              // geometry_mode "Triangle Mesh" / use_analytic_intersections=false (VulkanRayTracer.cpp:226-250)
    int rtaoGeometry = 0;                     // rtao_geometry: 0 = auto (the reference's triangle tubes once lv_set_tube_triangle_mesh was called), 1 = capsules, 2 = triangle_tubes
    bool useMlat = false;                     // VulkanRayTracer.hpp:133
    uint32_t mlatNumNodes = 8;                // :134
    uint32_t mlabNumLayers = 8;               // mlab_num_layers: numLayers of rendering mode 3, 1 ... 64 (MLABRenderer.cpp:133-135,330)
    uint32_t mboitNumMoments = 4;             // mboit_num_moments: 4 | 6 | 8 power moments of rendering mode 6 (MBOITRenderer.cpp:41-45)
    float mboitOverestimation = 0.1f;         // mboit_overestimation: overestimationBeta in [0, 1] (MBOITRenderer.cpp:45,609)
    float mboitMomentBias = 0.0f;             // mboit_moment_bias: 0 = auto (5e-7 / 5e-6 / 5e-5 for 4 / 6 / 8, MBOITRenderer.cpp:136-145), else (0, 0.1]
    uint32_t al64NumLayers = 8;               // atomic_loop_num_layers: numLayers of rendering mode 10, 1 ... 64 (AtomicLoop64Renderer.hpp:112)
    bool wboitOpenglWeight = false;           // wboit_depth_weight: false = "reference" (default, WBOITGather.glsl:23), true = "opengl" (the commented line)
    uint32_t peelMaxLayers = 2000;            // depth_peeling_max_layers: the cap of rendering mode 9's passes, 1 ... 2000 (DepthPeelingRenderer.cpp:288)
    uint32_t dcMaxColour = 0;                 // depth_complexity_max_colour: 0 = auto (numFragmentsMaxColor from the frame's maximum), else that value
    bool mboitStreamed = false;               // mboit_fragment_storage: false = "pool" (default), true = "streamed" (k_mboit_stream_pass: no fragment pool)
    bool lineQuads = false;                   // line_primitive_mode: false = "Tube (Programmable Pull)", true = "Quads (Programmable Pull)" (lv_linequad.h)
    // the simulation-mesh hull (lv_hull.h): hull_opacity (0.3, LineData.hpp:474; hullOpacitySet: the key has been set -- the reference's
    // shallRenderSimulationMeshBoundary is false until the setting arrives, LineData.cpp:142-145), hull_color (the linear value of sRGB
    // 0.5, LineData.hpp:472-473), hull_use_shading (:475)
    float hullOpacity = 0.3f;
    bool hullOpacitySet = false;
    float hullColor[3] = {0.214041144f, 0.214041144f, 0.214041144f};
    bool hullUseShading = true;
    // EAW denoiser of the RTAO pass (ambient_occlusion_denoiser; AO defaults of createDenoiserObject, Denoiser.cpp:54-62)
    bool eawEnabled = false;
    uint32_t eawIterations = 3;               // eaw_denoiser_iterations (GUI range 0..5, EAWDenoiser.cpp:437)
    bool eawColorWeights = true, eawPositionWeights = true, eawNormalWeights = true;
    float eawPhiColor = 0.49f, eawPhiPosition = 0.3f, eawPhiNormal = 0.1f;
    bool eawUseSharedMemory = true;           // true: EAWDenoise.Compute (default), false: EAWDenoise.Fragment
    // ambient_occlusion_denoiser = "SVGF" (Denoiser.hpp:65).  The reference exposes these in the GUI only (SVGF.cpp:427-436,
    // SVGF.hpp:70-72,115); the svgf_denoiser_* keys are this build's.
    // band data (ribbons): use_ribbons / thick_bands / min_band_thickness (LineDataFlow.cpp:587-606), band_width
    // (LineRenderer.cpp:442-449, STANDARD_BAND_WIDTH DataSetList.hpp:47), min band thickness LineData.cpp:54; the ray tracer's
    // "Elliptic Tubes" switch has no settings key in the reference (VulkanRayTracer.cpp:198-201): use_analytic_elliptic_tubes
    bool useRibbons = false, thickBands = true, ellipticTubes = false;
    float bandWidth = 0.005f, minBandThickness = 0.15f;
    // rotating helicity bands of flow lines with a helicity attribute: rotating_helicity_bands, separator_width (0.2,
    // LineDataFlow.cpp:54), band_subdivisions (6, LineDataFlow.hpp:188), helicity_rotation_factor (1, :171); settings keys :601-624
    bool helicityBands = false, uniformTwistLineWidth = true; // use_uniform_twist_line_width, LineDataFlow.cpp:53
    float separatorWidth = 0.2f, helicityRotationFactor = 1.0f;
    bool useTwistLineTexture = false;         // use_twist_line_texture (USE_HELICITY_BANDS_TEXTURE once a texture is loaded, LineDataFlow.cpp:2437)
    uint32_t twistFilterMode = 5;             // twist_line_texture_filtering_mode[_index]: "Linear Mipmap Linear" (LineDataFlow.hpp default)
    uint32_t bandSubdivisions = 6;
    bool svgfEnabled = false;
    uint32_t svgfIterations = 5;              // maxNumIterations, SVGF.hpp:115 (GUI range 0..5)
    float svgfAllowedZDist = 0.002f, svgfAllowedNormalDist = 0.02f; // SVGF.hpp:70-71
    // ambient_occlusion_denoiser = "Spatial Hashing" (Denoiser.hpp:64).  GUI-only in the reference (SpatialHashingDenoiser.cpp:89-92,
    // 184-186, .hpp:101); the spatial_hashing_* keys are this build's.
    bool shEnabled = false;
    float shSp = 8.0f;                        // spatial_hashing_s_p: cell size in pixels, 0.1 ... 20
    int shSMinExp = -17;                      // spatial_hashing_s_min_exp: s_min = 10^exp, -20 ... -1
    float shSNd = 3.0f;                       // spatial_hashing_s_nd: normal coarseness, 1 ... 10
    uint32_t shNumCells = 10000000u;          // spatial_hashing_num_cells (hm_cells, SpatialHashingDenoiser.cpp:42), >= 10
    // intersection_form: 0 = auto (default): the reference's literal roots whenever the RTAO pass traces the reference's
    // triangle tubes (rtao_geometry = triangle_tubes: the colour pass is then the only user of the capsule test and the
    // literal form is nearly free), closest approach otherwise; 1 = closest_approach; 2 = literal
    int intersectionForm = 0;
    // ppll_fragment_source: 0 = auto (default): raster_prism for plain flow lines, capsule_entry for band data / helicity bands
    // (not built for the prism yet); 1 = capsule_entry (entry hits of the pixel-centre ray against the analytic
    // capsules: the probe of rounds 1-3); 2 = raster_prism (the rasterised N-gon prism of the reference's default primitive mode)
    int ppllFragmentSource = 0;
    // ppll_prism_rasteriser: false = "segments" (default: one lane per line segment over its screen rectangle, k_ppll_raster_prism),
    // true = "lbvh" (the all-hits walk of the viewing rays through the segment LBVH, k_ppll_gather<LV_PRIM_PRISM>); same fragments
    bool ppllPrismLbvhWalk = false;
    bool ppllRayTracerColour = false;         // ppll_fragment_colour: false = "raster" (the reference's gather shader, default), true = "ray_tracer"
    bool mlatRecordTrace = false;             // with collect_stats: record every pixel's candidate visiting order
    uint32_t mlatTraceCapacity = 1u << 22;    // records (16 B each)
    bool hullRayTracing = false;              // hull_ray_tracing: false = "off" (default: mode 11 refuses a drawn hull), true = "on" (lv_hull_rt.h)
    bool rtRecordHits = false;                // rt_record_hits: a whole-viewport mode-11 frame records every step of every pixel's loop (lv_rt_get_hits)
    uint32_t rtHitsCapacity = 1u << 22;       // rt_hits_capacity: records (36 B each)
    bool hullFragmentPool = false;            // hull_fragment_pool: false = "off" (default: modes 2 and 3 refuse a drawn hull), true = "on" (lv_hull_pool.h)
};

struct LvMulti;
struct lv_ctx {
    LvMulti* multi = nullptr;                 // lv_create_multi: the ranks this handle drives (lv_multi.hip); null = one device
    int device = 0;
    int numCUs = 256;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    std::string lastError;

    // scene
    uint32_t numPoints = 0, numSegs = 0, numNodes = 0;
    LvDeviceBuffer points, segIdx;            // input order
    LvDeviceBuffer nodes, segs, segAxis, leafSeg, segToLeaf; // accel
    LvDeviceBuffer prismFrames;               // per leaf: the frames of the segment's two line points (lv_prism.h), 64 B
    LvDeviceBuffer tf;
    uint32_t tfN = 0;
    float attrMin = 0.0f, attrMax = 1.0f;
    bool accelValid = false;
    float accelLineWidth = -1.0f;
    uint32_t bvhDepth = 0, wideDepth = 0;     // height of the binary LBVH (reported) / levels of the 4-wide tree (stack size)
    // triangle tubes (RTAO geometry of the reference), own LBVH
    uint32_t numTris = 0, numTriVerts = 0, numTriPoints = 0, numTriNodes = 0, triBvhDepth = 0, triWideDepth = 0;
    LvDeviceBuffer triIdx, triVerts, triPoints; // input order
    LvDeviceBuffer triNodes, tris;              // accel
    LvDeviceBuffer triPairFlag;                 // k_tri_pairs_check's verdict
    // the simulation-mesh hull (lv_set_hull_mesh): 3 indices per triangle, 32-B HullTriangleVertexData; it does not belong to the lines
    LvDeviceBuffer hullIdx, hullVerts;
    uint32_t hullNumTris = 0, hullNumVerts = 0;
    // its LBVH for the ray tracer (lv_bvh_build_hull; hull_ray_tracing, lv_trace_rays_hull): 48-B triangle records, one per leaf.  The
    // pad of lv_ray_triangle's own-box rule depends on the mesh alone, so only lv_set_hull_mesh invalidates the tree
    LvDeviceBuffer hullNodes, hullTris;
    uint32_t hullNumNodes = 0, hullBvhDepth = 0, hullWideDepth = 0;
    float hullMaxAbs = 0.0f, hullPad = 0.0f;  // largest |coordinate| of the mesh (lv_set_hull_mesh); hullPad of lv_hull_rt.h from it
    bool hullAccelValid = false;
    LvDeviceBuffer rtHits;                    // rt_record_hits: 9-word records of the last recording frame
    bool rtHitsValid = false;                 // the last frame was a whole-viewport mode-11 frame that recorded
    uint32_t rtHitsFrameCapacity = 0;         // ... into this many records (rt_hits_capacity may have changed since)
    bool triLeafPairs = false;                  // the leaves of the triangle LBVH as built hold 64-B pair records
    bool triMeshSet = false, triAccelValid = false;
    // lv_set_trajectories (lv_lines.hip): the trajectories themselves in HBM; `points` / `segIdx` are then written by the a2 kernels and
    // the tube mesh is tessellated on the device whenever a frame needs it at another line width / subdivision count
    LvDeviceBuffer trajPos, trajAttr, trajOff;      // 3 floats / 1 float per point, numLines + 1 offsets
    LvDeviceBuffer trajLineValid, trajLineRef, trajRecLine, trajTess; // per line: valid points, LvLineRef; per record: its line; tessellation offsets + tables
    uint32_t trajNumLines = 0, trajNumPoints = 0;
    bool trajHasAttr = false, trajSet = false;
    // lv_set_trajectories_with_bands: ribbon directions (3 floats per point) and the helicity attribute (1 float per point, max |h| in
    // trajMaxHelicity's one float); per record: its trajectory point and the mesh table's rotation, which runs on across all lines
    // (computed once per data set).  trajPoints*: what the records in `points` carry (lv_ensure_line_points rewrites them on change)
    LvDeviceBuffer trajRibbon, trajHelicity, trajMaxHelicity, trajRecPoint, trajMeshRot;
    bool trajHasRibbons = false, trajHasHelicity = false;
    bool trajPointsRibbon = false, trajPointsHelicity = false;
    bool triMeshFromTraj = false;             // the mesh in triIdx / triVerts / triPoints was tessellated here (not passed by the caller)
    float triMeshLineWidth = -1.0f;
    uint32_t triMeshSubdivisions = 0;
    bool triMeshRibbons = false, triMeshHelicity = false;   // the rest of the device mesh's cache key (host/LineData.cpp:633-636)
    float triMeshBandWidth = -1.0f, triMeshMinBandThickness = -1.0f;
    float triAccelLineWidth = -1.0f, triPad = 0.0f;
    uint32_t triLeafSize = 1;                 // triangles per leaf of the triangle LBVH as built (opt.triLeafSize at build time)

    // static RTAO prebaker
    LvDeviceBuffer bakeBlendingWeights, bakeSamplingLocations, bakedAo, bakeLcgSkip;
    uint32_t bakeNumLineVertices = 0, bakeNumParametrizationVertices = 0;
    bool bakeParamSet = false, bakeValid = false;
    // asynchronous bake (lv_bake_ao_start): the table is computed on a second stream with scratch buffers of its own while frames keep
    // rendering on the context's stream; lv_bake_ao_poll / the next frame adopt it once the stream has finished
    hipStream_t bakeStream = nullptr;
    hipEvent_t evBakePrereq = nullptr, evBakeDone = nullptr;
    bool bakeAsyncPending = false;            // a bake is queued / running on bakeStream
    uint64_t bakeGeneration = 0, bakePendingGeneration = 0; // bumped by everything that invalidates a table
    LvDeviceBuffer bakedAoPending, bakeCounters, bakeGbuf, bakeSamples, bakeOverflow;
    std::vector<uint32_t> bakeSkipHost;       // LCG skip-ahead table (source of an asynchronous upload: must outlive the call)
    uint32_t bakeSlotsHost = 0;

    // streamline tracing (lv_flow.hip)
    LvDeviceBuffer flowVectors, flowScalars, flowMisc, flowSeeds, flowOutPos, flowOutAtt, flowCounts;
    uint32_t flowXs = 0, flowYs = 0, flowZs = 0, flowNumScalars = 0;
    float flowDx = 1.0f, flowDy = 1.0f, flowDz = 1.0f, flowMaxMagnitude = 0.0f;
    bool flowGridSet = false;
    std::vector<float> flowPositions;                 // result of the last lv_trace_streamlines call (host side)
    std::vector<std::vector<float>> flowAttributes;
    std::vector<uint32_t> flowOffsets;
    std::vector<uint32_t> flowSeedIndex;              // per line: index of the seed point inside the merged line

    // camera
    bool cameraSet = false;
    float view[16] = {}, proj[16] = {}, invView[16] = {}, invProj[16] = {};
    float fovY = 0.0f, nearDist = 0.01f, farDist = 100.0f;
    uint32_t width = 0, height = 0;
    float background[4] = {1.0f, 1.0f, 1.0f, 1.0f};

    LvOptions opt;

    // frame resources
    LvDeviceBuffer depthMinMax;               // 2 floats (+2 encoded uints)
    LvDeviceBuffer ao;                        // width*height floats (the latest AO image)
    LvDeviceBuffer aoAlt;                     // second image of the halo mode's ping-pong accumulation (lv_run_ao)
    LvDeviceBuffer featNormal, featNormalAlt, featPosition, featPositionAlt; // EAW feature maps (float4 per pixel) + ping-pong
    LvDeviceBuffer eawPing, eawPong;          // a-trous passes
    const float* aoResult = nullptr;          // what the colour pass samples: ao (raw) or the denoised image
    bool aoRestart = false;                   // the denoiser changed: a progressive RTAO accumulation may only continue from frame 0
    LvSvgfState svgf;
    LvDeviceBuffer svgfGiven;                 // every image of one lv_svgf_denoise_buffers call (lv_svgf_denoise_given)
    LvDeviceBuffer fullFrameTile;             // one tile origin (0, 0): the SVGF and Spatial Hashing chains always cover the viewport
    LvShState sh[2];                          // spatial hashing: [0] the renderer's map, [1] the map of lv_spatial_hashing_denoise_buffers
    LvDeviceBuffer shMapCells, shMapCounters; // ... map 0: allocated while the denoiser is selected
    LvDeviceBuffer shGivenCells, shGivenCounters; // ... map 1
    LvDeviceBuffer shRead, shNormal, shPosition, shPing, shPong; // its read image, world-space maps {xyz, 0} and a-trous passes (full viewport)
    LvDeviceBuffer shGiven, shCompact;        // every image of one lv_spatial_hashing_denoise_buffers call; lv_spatial_hashing_get_cells' copy
    uint32_t aoGlobalFrameNumber = 0;         // RTAO iterations since lv_set_lines (globalFrameNumber, ...AmbientOcclusion.cpp:582)
    float lastFrameViewProj[16] = {};         // projection * view at the previous RTAO iteration (:456,631)
    bool lastFrameViewProjValid = false;
    uint32_t tilesHalo = 0;                   // halo the uploaded tilesHaloDev list was built for
    LvDeviceBuffer tilesHaloDev;              // tile origins - 1 (AO pass on dilated tiles)
    std::vector<uint32_t> tilesHaloHost;
    bool tilesHaloUploaded = false;
    uint32_t aoNumGroups = 0, aoGroupsPerTile = 0; // geometry of the last RTAO pass' per-group counters (aoList)
    LvDeviceBuffer aoGbuf, aoList, aoSamples; // RTAO wavefront buffers
    LvDeviceBuffer firstHit;                  // k_primary_pair: {t bits, (leaf << 2) | kind} of the colour pass' first ray per output pixel
    LvDeviceBuffer counters;                  // device counters (LvCounters + misc)
    LvDeviceBuffer ppllNodes, ppllStart, ppllCount, ppllScratch;
    LvDeviceBuffer prismRecords, scanTemp;    // raster_prism: {pixel, leaf | triangle, rank} records of the coverage kernel; k_ppll_scan: block totals, block bases, completion counter
    uint32_t ppllScanBlocks = 0;              // raster_prism: workgroups of the last k_ppll_scan (scanTemp = totals, bases, counter)
    LvDeviceBuffer twistTex;                  // twist-line texture: float4 texels, mip levels back to back
    uint32_t twistW = 0, twistH = 0, twistLevels = 0;
    LvDeviceBuffer flowOccupancy;             // max-helicity-first seeding: the occupancy grid, one byte per cell (grid-based check) / the list heads of the finished points' grid
    LvDeviceBuffer flowPoints, flowPointsNext; // point-based termination checks: finished points (12 B) and their per-cell list links
    size_t flowPointsCapacity = 0;
    LvDeviceBuffer flowSelfGrid;              // loop check "Grid": one bit per cell and line of a batch
    LvDeviceBuffer prismLeafList;             // raster_prism, sharded frames: segments that can touch the frame's tile list (k_ppll_cull_segments)
    LvDeviceBuffer ppllCoarse;                // raster_prism, sharded frames: 32 x 32-pixel cells that hold requested pixels (k_ppll_mark_tiles)
    LvDeviceBuffer hullRanks;                 // hull_fragment_pool: per padded pixel, the hull entries k_hull_shade_records has placed so far
    LvDeviceBuffer ppllOverflow;              // raster_prism: pixel addresses with more kept fragments than ppllMaxNumFrags (k_ppll_pixel_pass)
    LvDeviceBuffer mlabLong;                  // mode 3: {pixel address, output index} of the pixels k_mlab_resolve_long folds
    LvDeviceBuffer mlabStatsSnap;             // mode 3 with collect_stats: the statistics counters before the front end (pool regrowth)
    uint64_t mlabPoolSlots = 0;               // modes 3 and 6: fragment slots the largest frame so far needed (the pool never drops one)
    uint32_t mboitBoxOrd[6] = {0, 0, 0, 0, 0, 0};   // mode 6: k_mboit_points_box's result for the current line points (lv_bvh_build resets)
    bool mboitBoxValid = false;
    LvDeviceBuffer mboitAccum;                // mode 6, streamed storage: 1 + N moment sums and 4 colour sums of 8 B per padded pixel (addressed like ppllCount)
    LvDeviceBuffer al64Buf;                   // mode 10: K slots and 5 tail sums of 8 B per padded pixel (addressed like ppllCount)
    LvDeviceBuffer wboitBuf;                  // mode 8: 5 sums of 8 B per padded pixel (addressed like ppllCount)
    LvDeviceBuffer peelBuf, dcStatsDev;       // mode 9: 32 B per padded pixel (lv_peel_buffers); modes 5 and 9: the words of k_dc_reduce
    LvDeviceBuffer visBuf, deferredTf;        // mode 1: the visibility buffer, 8 B per padded pixel (addressed like ppllCount); the transfer function with alpha 1
    // The last frame, when it left per-pixel buffers behind that a *_get_* call reads: a streamed mode-6 frame (mboitAccum), a mode-8
    // (wboitBuf), mode-10 (al64Buf), mode-5 or mode-9 frame (ppllCount, peelBuf, dcStatsDev), a mode-1 frame (visBuf).  Each of these frame functions sets it;
    // lv_frame_render clears it at its top, and so does every resolve-only entry point (they overwrite ppllCount and the counters).
    struct StreamedFrame {
        int mode = 0;                         // 0: none; else LV_RENDERING_MODE_* (1, 5, 6, 8, 9 or 10)
        bool full = false;                    // the frame covered the whole viewport
        uint32_t w = 0, h = 0;                // its viewport
        uint32_t tile[2] = {0, 0};            // its ppll tile
        uint32_t param = 0;                   // mode 6: the moment count N; mode 10: the layer count K
        // modes 5, 8, 10: the line pass drew line quads.  lv_line_quads_get_fragments evaluates the pass again on the context's resident
        // line data and AO image, so it also asks that these are still the frame's: the segment count and whether the lighting read the
        // AO image, as recorded here
        bool quads = false;
        uint32_t quadsSegs = 0;
        bool quadsAo = false;
    } streamed;
    bool ppllArrays = false;                  // the last PPLL frame left per-pixel runs (raster_prism), not linked lists
    LvDeviceBuffer tilesDev, outDev, scratchRays, stackOverflow, mlatTrace;
    LvDeviceBuffer selftestIn, selftestOut;   // lv_selftest_eval: argument and result words
    LvDeviceBuffer accum;                     // rgba8 of the previous accumulated frame (full viewport)
    uint32_t* pinned = nullptr;               // 64 B of pinned host memory for small read-backs (hipHostMalloc)
    LvDeviceBuffer partitionScratch;          // accel_partition = sah: leaf states, path codes, cluster tables and bins of the build, kept between builds like buildArena
    LvDeviceBuffer buildArena;                // temporaries of the LBVH builds, kept between builds
    // dispatch order of the 64x64-pixel groups of the tile kernels (lv_group_order_prepare): [0] colour pass, [1] RTAO pass geometry
    struct GroupOrder {
        LvDeviceBuffer cost, order;
        uint32_t n = 0, tileW = 0, tileH = 0;
        uint64_t generation = ~0ull;
        bool active = false;                  // in use by the frame being queued
    } groupOrder[2];
    bool groupOrderSorted = false;            // this frame's k_group_order is queued
    uint64_t tilesGeneration = 0;             // bumped whenever tilesDev receives another list
    bool tilesCoverViewport = false;          // the uploaded tile list covers every pixel of the viewport (key: width, height, tile size)
    uint32_t tilesCoverKey[4] = {0, 0, 0, 0};
    bool tilesOverlap = false;                // two tiles of the uploaded list share a pixel (same key): the RTAO running mean must not update in place
    std::vector<uint32_t> tilesHost;          // staging copy: caller's tile list is borrowed for the call only
    bool tilesUploaded = false;               // tilesDev holds tilesHost
    uint64_t ppllPoolNodes = 0;               // physical node slots of the pool (logical size + per-wave chunk slack)
    // viewport the per-frame buffers were last rendered with (read-backs copy these extents, not the current camera's)
    uint32_t aoW = 0, aoH = 0, ppllPaddedW = 0, ppllPaddedH = 0, accumW = 0, accumH = 0;

    // stats
    lv_stats stats;
    hipEvent_t ev[16];
    bool evCreated = false;
    bool evBuildValid = false, evFrameValid = false, evPhaseRecorded = false;
    bool evTriBuildValid = false;             // ev[14], ev[15] bracket the last triangle-LBVH build
    bool evLinePointsValid = false, evTessValid = false; // ev[4], ev[6]: the a2 kernels of lv_set_trajectories; ev[8], ev[9]: the last device tessellation
    int lastMode = 0;
    // per-kernel launch timers: ring of event pairs per kernel id (LV_KERNEL_*)
    static constexpr int kNumKernels = 12;    // LV_KERNEL_SH_TAIL is the last; lv_stats reports the first eight
    static constexpr int kRing = 512;
    hipEvent_t evKernel[kNumKernels][2 * kRing];
    uint64_t kernelLaunches[kNumKernels] = {};
};

int lv_fail(lv_ctx* ctx, int code, const char* fmt, ...);
// width the capsule LBVH's leaf boxes are padded with: the band width for elliptic tubes (useRibbonNormals,
// LineDataFlow.cpp:2120-2126), the line width otherwise
// RTAO geometry of the frame: the reference's triangle tubes (VulkanRayTracedAmbientOcclusion traces nothing else) whenever the mesh
// is there, the analytic capsules of the colour pass otherwise / on request
inline bool lv_ao_triangle_tubes(const lv_ctx* ctx) {
    return ctx->opt.rtaoGeometry == 2 || (ctx->opt.rtaoGeometry == 0 && (ctx->triMeshSet || ctx->trajSet));
}
// the capsule roots in use: the reference's textbook form (RayIntersectionTestsVulkan.glsl:39-119) -- the default -- or the
// closest-approach form; "auto" leaves the reference's form only where this build traces AO rays against the analytic capsules
// (a mode the reference does not have: rays that start on a capsule need the stable roots)
inline bool lv_literal_intersection(const lv_ctx* ctx) {
    if (ctx->opt.intersectionForm != 0) return ctx->opt.intersectionForm == 2;
    return !(ctx->opt.useAmbientOcclusion && !ctx->opt.aoPrebaked && !lv_ao_triangle_tubes(ctx));
}
// LineData::shallRenderSimulationMeshBoundary: a mesh is set and hull_opacity has been set to a value > 0
inline bool lv_hull_drawn(const lv_ctx* ctx) {
    return ctx->hullNumTris != 0u && ctx->opt.hullOpacitySet && ctx->opt.hullOpacity > 0.0f;
}
// a mode-11 frame's colour pass is k_render_rt_hull (lv_hull_rt.hip): hull_ray_tracing = on while a hull is drawn, or a recording frame
inline bool lv_rt_hull_kernel(const lv_ctx* ctx) {
    return !ctx->opt.useMlat && ((ctx->opt.hullRayTracing && lv_hull_drawn(ctx)) || ctx->opt.rtRecordHits);
}
inline float lv_accel_width(const lv_ctx* ctx) {
    return (ctx->opt.useRibbons && ctx->opt.ellipticTubes) ? ctx->opt.bandWidth : ctx->opt.lineWidth;
}

#define LV_HIP(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return lv_fail(ctx, LV_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

int lv_buf_reserve(lv_ctx* ctx, LvDeviceBuffer& b, size_t bytes);
// event pair of the next launch of kernel `id`
inline hipEvent_t lv_kernel_ev(lv_ctx* ctx, int id, int which) {
    return ctx->evKernel[id][2 * (ctx->kernelLaunches[id] % lv_ctx::kRing) + which];
}
#define LV_TIMED_LAUNCH(ctx, id, launch)                                      \
    do {                                                                      \
        const bool lvTimed = (((ctx)->opt.timerMask >> (id)) & 1u) != 0u;     \
        if (lvTimed) LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, id, 0), (ctx)->stream)); \
        launch;                                                               \
        if (lvTimed) {                                                        \
            LV_HIP(ctx, hipEventRecord(lv_kernel_ev(ctx, id, 1), (ctx)->stream)); \
            (ctx)->kernelLaunches[id]++;                                      \
        }                                                                     \
    } while (0)
void lv_buf_free(LvDeviceBuffer& b);

// lv_bvh.hip
int lv_bvh_build(lv_ctx* ctx);
int lv_bvh_build_triangles(lv_ctx* ctx);
int lv_bvh_build_hull(lv_ctx* ctx);
// lv_lines.hip: (re)tessellates the tube mesh of lv_set_trajectories' lines if the line width / subdivision count / band settings
// changed; no-op otherwise
int lv_ensure_tube_mesh(lv_ctx* ctx);
// lv_lines.hip: rewrites lv_set_trajectories' line points if use_ribbons + use_analytic_elliptic_tubes (ribbon normals) or
// rotating_helicity_bands (lineRotation) changed since they were written; no-op otherwise
int lv_ensure_line_points(lv_ctx* ctx);
// lv_multi.hip: one frame over the GPUs of a node behind the same handle
int lv_multi_create(lv_ctx* handle, const int* devices, int numDevices, const char* transport);
void lv_multi_destroy(lv_ctx* handle);
int lv_multi_num_ranks(const lv_ctx* handle);
lv_ctx* lv_multi_rank(lv_ctx* handle, int r);
int lv_multi_render(lv_ctx* handle, int mode, const uint32_t* tilesXY, uint32_t numTiles, uint32_t tileW, uint32_t tileH, bool image,
                    uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* outDevice);
int lv_multi_render_rect(lv_ctx* handle, int mode, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* outDevice);
int lv_multi_rebalance_impl(lv_ctx* handle, double baseCostPerTile);
int lv_multi_get_deal(lv_ctx* handle, uint32_t* outOwner, uint32_t capacity, uint32_t* outCount);
// repeats a setter on the other ranks of a multi-device handle (no-op for a single-device context)
template <class F>
inline int lv_forward_to_ranks(lv_ctx* handle, F&& f) {
    const int n = lv_multi_num_ranks(handle);
    for (int r = 1; r < n; r++) {
        lv_ctx* p = lv_multi_rank(handle, r);
        const int rc = f(p);
        if (rc) return lv_fail(handle, rc, "rank %d (device %d): %s", r, p->device, p->lastError.c_str());
    }
    // the setters select their rank's device: leave the calling thread on the handle's (outputs live on the first device)
    if (n > 1) (void)hipSetDevice(handle->device);
    return LV_OK;
}
// lv_mlat.hip
struct LvUniforms;
struct LvSceneDev;
struct LvTiles;
int lv_mlat_render(lv_ctx* ctx, const LvUniforms& U, const LvSceneDev& S, const LvTiles& T, uint32_t gridTiles,
                   uint32_t* out, LvDevCounters* dc, bool triangles);
// lv_render.hip
int lv_frame_render(lv_ctx* ctx, int mode, const uint32_t* tilesXYHost, uint32_t numTiles, uint32_t tileW,
                    uint32_t tileH, void* outDevice);
int lv_frame_trace_rays(lv_ctx* ctx, const float* o, const float* d, float tMin, float tMax, uint32_t n, float* outT,
                        uint32_t* outSeg, uint32_t* outKind);
int lv_frame_trace_rays_triangles(lv_ctx* ctx, const float* o, const float* d, float tMin, float tMax, uint32_t n,
                                  float* outT, uint32_t* outTri, float* outUV);
int lv_frame_trace_rays_hull(lv_ctx* ctx, const float* o, const float* d, float tMin, float tMax, uint32_t n, float* outT,
                             uint32_t* outTri, float* outUV);
// inFrame: called by lv_frame_render, which reserved the traversal-stack slab for the bake too (nothing inside a frame moves it)
int lv_bake_ambient_occlusion(lv_ctx* ctx, bool async = false, bool inFrame = false);
int lv_bake_poll(lv_ctx* ctx, bool wait);
// everything that changes what a baked table depends on: a running asynchronous bake still reads the old inputs, so it is waited for
// (and its result discarded: the generation no longer matches)
inline void lv_invalidate_bake(lv_ctx* ctx) {
    if (ctx->bakeAsyncPending) (void)hipEventSynchronize(ctx->evBakeDone);
    ctx->bakeValid = false;
    ctx->bakeGeneration++;
}
int lv_frame_depth_range(lv_ctx* ctx);
int lv_frame_mlab_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w,
                               uint32_t h, uint8_t* out);
int lv_frame_mboit_stream_moments(lv_ctx* ctx, float* out, uint64_t capacityFloats);
int lv_mboit_stream_overflow(lv_ctx* ctx);
int lv_frame_wboit_buffers(lv_ctx* ctx, int64_t* outSums, uint32_t* outCounts, uint64_t capacityPixels);
int lv_frame_wboit_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w, uint32_t h,
                                uint8_t* out, int64_t* outSums);
int lv_frame_peel_buffers(lv_ctx* ctx, int mode, float* outAccum, uint32_t* outLayers, uint32_t* outCounts, uint64_t capacityPixels);
int lv_frame_dc_stats(lv_ctx* ctx, uint64_t out[5]);
int lv_frame_peel_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w, uint32_t h,
                               uint8_t* out, float* outAccum, uint32_t* outLayers);
int lv_frame_deferred_buffers(lv_ctx* ctx, uint32_t* outPrimitive, float* outDepth, uint64_t capacityPixels);
int lv_frame_deferred_shade_only(lv_ctx* ctx, const uint32_t* primitive, const float* depth, uint32_t w, uint32_t h, uint32_t* out);
int lv_frame_line_quads_fragments(lv_ctx* ctx, uint32_t* outPixel, uint32_t* outSegment, uint32_t* outTriangle, float* outDepth, float* outRgba,
                                  uint64_t capacity, uint64_t* outCount);
int lv_frame_hull_fragments(lv_ctx* ctx, uint32_t* outPixel, uint32_t* outTriangle, float* outDepth, float* outRgba, uint64_t capacity,
                            uint64_t* outCount);
int lv_frame_al64_num_layers(lv_ctx* ctx, uint32_t* out);
int lv_frame_al64_buffers(lv_ctx* ctx, uint64_t* outSlots, uint64_t* outTail, uint64_t capacityPixels);
int lv_frame_al64_resolve_only(lv_ctx* ctx, const uint64_t* keys, uint64_t numKeys, const uint64_t* offsets, uint32_t w, uint32_t h,
                               uint8_t* out, uint64_t* outSlots, uint64_t* outTail);
int lv_frame_mboit_resolve_only(lv_ctx* ctx, const uint32_t* entries, uint64_t numEntries, const uint64_t* offsets, uint32_t w,
                                uint32_t h, float logDepthMin, float logDepthMax, float* outMoments, uint8_t* out);
int lv_frame_ppll_resolve_only(lv_ctx* ctx, const uint32_t* nodes, uint64_t numNodes, const uint32_t* start,
                               uint64_t numPixels, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint8_t* out);
void lv_fill_uniforms(const lv_ctx* ctx, LvUniforms& U);
bool lv_ppll_prism_source(const lv_ctx* ctx);
// lv_svgf.hip
int lv_svgf_prepare(lv_ctx* ctx);
int lv_svgf_denoise(lv_ctx* ctx, LvSvgfState& V, uint32_t width, uint32_t height, const float* noisy);
int lv_svgf_denoise_given(lv_ctx* ctx, uint32_t w, uint32_t h, const float* noisy, const float* normalDepth, const float* flowFwidth,
                          float* colorHistory, float* momentsHistory, float* normalDepthHistory, float* out);
// lv_sh.hip: the spatial-hashing denoiser; `which` = index into ctx->sh
int lv_sh_denoise_frame(lv_ctx* ctx, const float camPos[3], const uint32_t* tileBase, uint32_t numGroups, uint32_t tileW, uint32_t tileH,
                        uint32_t groupsX, uint32_t groupsPerTile, const uint32_t* hitCount, uint64_t maxPixels, const float** result);
int lv_sh_denoise_given(lv_ctx* ctx, uint32_t w, uint32_t h, const float* noisy, const float* normalWorld, const float* positionWorld,
                        const float camPos[3], float* outRead, float* out);
int lv_sh_reset(lv_ctx* ctx, int which);
int lv_sh_release(lv_ctx* ctx, int which);
int lv_sh_get_stats(lv_ctx* ctx, int which, uint64_t out[4]);
int lv_sh_get_cells(lv_ctx* ctx, int which, uint64_t* keys, uint64_t* accumulators, uint64_t capacity, uint64_t* outCount);
// lv_render.hip: the a-trous tail of the spatial-hashing denoiser -- three passes of k_eaw_pass<true> over a w x h image with the
// settings of SpatialHashingDenoiser.cpp:82-87; *result = the buffer that holds the last pass
int lv_eaw_tail(lv_ctx* ctx, uint32_t w, uint32_t h, const float* src, const float4* normalMap, const float4* positionMap, float* ping,
                float* pong, const float** result);
// what the renderer's map was accumulated from has changed (lines, line width): the next denoise starts from an empty map
inline void lv_sh_invalidate(lv_ctx* ctx) { ctx->sh[0].clearPending = true; }
// lv_flow.hip
int lv_flow_set_grid(lv_ctx* ctx, const float* vectorField, uint32_t xs, uint32_t ys, uint32_t zs, float dx, float dy,
                     float dz, const float* const* scalarFields, uint32_t numScalarFields);
int lv_flow_trace(lv_ctx* ctx, const float* seeds, uint32_t numSeeds, const lv_streamline_settings* settings);
int lv_flow_trace_max_helicity_first(lv_ctx* ctx, const float* helicityField, const lv_streamline_settings* settings,
                                     const lv_helicity_seeding_settings* seeding);
float lv_mat4_inverse(const float* m, float* inv);   // returns the determinant
void lv_mat4_mul(const float* A, const float* B, float* out);
