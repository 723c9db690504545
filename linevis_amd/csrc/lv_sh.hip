// lv_sh.hip -- spatial-hashing denoiser of the RTAO pass (ambient_occlusion_denoiser = "Spatial Hashing"); semantics: lv_sh.h.
//
//   k_sh_begin         the conditional clear of the map (occupied > numCells / 2, or forced by the host) and of its counters
//   k_sh_write         SH_Denoise.Compute-Write (glsl:248-334), order-independent: one lane per hit
//   k_sh_read          SH_Denoise.Compute-Read  (glsl:365-440): one lane per hit, <= 40 16-byte loads, no atomics
//   k_sh_scatter_maps  the world-space normal / position maps of the a-trous tail, from the same hit records
//   k_sh_given_records hit records from caller-supplied maps (lv_spatial_hashing_denoise_buffers)
//   lv_sh_denoise_*    Spatial_Hashing_Denoiser::denoise(), SpatialHashingDenoiser.cpp:104-133; the tail is lv_eaw_tail (lv_render.hip)
//
// Atomics (MI355X): every atomic is resolved in L2 and costs a round trip there; one that returns a value also holds its lane until
// the value is back.  The write pass issues no returning atomic but the CAS of a claim -- once per cell and clear -- and one atomicAdd
// per hit and level.  Combining the equal keys of a wave first (a ballot loop: leader = lowest pending lane, its key broadcast, the
// matching lanes' q summed with ballots, one atomicAdd per distinct key) was built and measured on the c3c frame and lost: a wave of
// k_ao_primary holds the pixels (W & 7, W >> 3) of the 64 8 x 8 cells of its group (lv_tile.h), i.e. pixels 8 apart, and the normal is
// part of the key, so a wave holds 56.0 distinct keys per level of 64 possible; the loop saved 12.5 % of the atomicAdds and cost more
// than they do (k_sh_write 0.329 ms with it, 0.286 ms without; DESIGN.md 6, EXPERIMENTS.md 24).
#include "lv_internal.h"
#include "lv_sh.h"
#include "lv_tile.h"

#include <cmath>

namespace {

inline uint32_t nblocks(uint64_t n) { return uint32_t((n + LV_BLOCK - 1) / LV_BLOCK); }

// the hits of a pass: G-buffer records (3 x float4: g0.xyz position, g1.w pixel bits, g2.xyz normal) addressed by compacted ordinal
struct LvShHits {
    const float4* gbuf;
    const uint32_t* tileBase;   // nullptr: record = ordinal
    uint32_t numGroups;
    LvAoLayout layout;
    const uint32_t* count;      // device count of ordinals (the RTAO pass' dc->aoCount), or nullptr: countImm
    uint32_t countImm;
};

__device__ __forceinline__ bool lv_sh_hit(const LvShHits& H, uint32_t ordinal, f3& position, f3& normal, uint32_t& pix) {
    const uint32_t count = H.count ? *H.count : H.countImm;
    if (ordinal >= count) return false;
    const size_t slot = lv_ao_slot(H.tileBase, H.numGroups, H.layout, ordinal);
    const float4 g0 = H.gbuf[3 * slot], g1 = H.gbuf[3 * slot + 1], g2 = H.gbuf[3 * slot + 2];
    position = mk3(g0.x, g0.y, g0.z);
    normal = mk3(g2.x, g2.y, g2.z);
    pix = __float_as_uint(g1.w);
    return !(normal.x == 0.0f && normal.y == 0.0f && normal.z == 0.0f);
}

__device__ __forceinline__ uint32_t lv_sh_wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) v += uint32_t(__shfl_xor(v, ofs, 64));
    return v;
}

// Every block reads the decision before any block changes what it is made from: the counters are rewritten by the block that takes the
// last ticket, i.e. after all blocks have read them and cleared their share.
__global__ __launch_bounds__(LV_BLOCK) void k_sh_begin(LvShCell* __restrict__ cells, uint32_t numCells, LvShCounters* c, uint32_t force) {
    const bool clear = force != 0u || c->occupied > numCells / 2u;
    if (clear) {
        ulonglong2* p = reinterpret_cast<ulonglong2*>(cells);
        for (size_t i = size_t(blockIdx.x) * LV_BLOCK + threadIdx.x; i < numCells; i += size_t(gridDim.x) * LV_BLOCK)
            p[i] = make_ulonglong2(0ull, 0ull);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        __threadfence();
        if (atomicAdd(&c->ticket, 1u) == gridDim.x - 1u) {
            if (clear) { c->occupied = 0u; c->stored = 0ull; c->dropped = 0ull; c->clears += 1u; }
            c->ticket = 0u;
        }
    }
}

__global__ __launch_bounds__(LV_BLOCK) void k_sh_write(const LvShHits H, const LvShParams P, const float* __restrict__ noisy,
                                                       LvShCell* cells, LvShCounters* c) {
    const uint32_t ordinal = blockIdx.x * LV_BLOCK + threadIdx.x;
    f3 position = mk3(0.0f, 0.0f, 0.0f), normal = position;
    uint32_t pix = 0u;
    float swd = 0.0f;
    // no lane leaves before the end: the sums below are the whole wave's
    const bool valid = lv_sh_hit(H, ordinal, position, normal, pix) && lv_sh_cell_size(P, position, swd);
    if (!__any(valid)) return;
    uint32_t stored = 0u, dropped = 0u, claimed = 0u;
    if (valid) {
        const float occlusion = fminf(fmaxf(noisy[pix], 0.0f), 1.0f);
        const unsigned long long word = ((unsigned long long)uint32_t(floorf(occlusion * 100.0f + 0.5f)) << LV_SH_COUNT_BITS) | 1ull;
        const LvShNormal n = lv_sh_normal(P, normal);
        for (int l = 0; l < LV_SH_LEVELS; l++) {
            const unsigned long long key = lv_sh_key(P, position, n, swd * float(1 << l));
            bool done = false;
            for (uint32_t i = 0; i < LV_SH_PROBES && !done; i++) {
                LvShCell* cell = cells + lv_sh_slot(key, i, P.numCells);
                unsigned long long cur = __atomic_load_n(&cell->key, __ATOMIC_RELAXED);
                if (cur == 0ull) {
                    cur = atomicCAS(&cell->key, 0ull, key);
                    if (cur == 0ull) { cur = key; claimed++; }
                }
                if (cur == key) {
                    atomicAdd(&cell->acc, word);
                    done = true;
                }
            }
            if (done) stored++; else dropped++;
        }
    }
    // one atomicAdd per wave and counter, none returning
    stored = lv_sh_wave_sum_u32(stored); dropped = lv_sh_wave_sum_u32(dropped); claimed = lv_sh_wave_sum_u32(claimed);
    if (lv_lane() == 0u) {
        if (stored) atomicAdd(&c->stored, (unsigned long long)stored);
        if (dropped) atomicAdd(&c->dropped, (unsigned long long)dropped);
        if (claimed) atomicAdd(&c->occupied, claimed);
    }
}

__global__ __launch_bounds__(LV_BLOCK) void k_sh_read(const LvShHits H, const LvShParams P, const LvShCell* __restrict__ cells,
                                                      float* __restrict__ out) {
    const uint32_t ordinal = blockIdx.x * LV_BLOCK + threadIdx.x;
    f3 position, normal;
    uint32_t pix;
    float swd;
    if (!lv_sh_hit(H, ordinal, position, normal, pix) || !lv_sh_cell_size(P, position, swd)) return;
    const LvShNormal n = lv_sh_normal(P, normal);
    uint32_t samples = 0u;
    float ao = 0.0f;
    for (int l = 0; l < LV_SH_LEVELS; l++) {
        const unsigned long long key = lv_sh_key(P, position, n, swd * float(1 << l));
        for (uint32_t i = 0; i < LV_SH_PROBES; i++) {
            const ulonglong2 cell = *reinterpret_cast<const ulonglong2*>(cells + lv_sh_slot(key, i, P.numCells));
            if (cell.x == 0ull) break;
            if (cell.x == key) {
                samples += uint32_t(cell.y & LV_SH_COUNT_MASK);
                ao += float(cell.y >> LV_SH_COUNT_BITS) / 100.0f;
                break;
            }
        }
        if (samples >= LV_SH_MIN_SAMPLES) break;
    }
    out[pix] = samples > 0u ? ao / float(samples) : 0.0f;
}

__global__ __launch_bounds__(LV_BLOCK) void k_sh_scatter_maps(const LvShHits H, float4* __restrict__ normalMap,
                                                              float4* __restrict__ positionMap) {
    const uint32_t ordinal = blockIdx.x * LV_BLOCK + threadIdx.x;
    f3 position, normal;
    uint32_t pix;
    if (!lv_sh_hit(H, ordinal, position, normal, pix)) return;
    normalMap[pix] = make_float4(normal.x, normal.y, normal.z, 0.0f);
    positionMap[pix] = make_float4(position.x, position.y, position.z, 0.0f);
}

// one record per pixel, in pixel order; a miss keeps its zero normal and is skipped by lv_sh_hit
__global__ __launch_bounds__(LV_BLOCK) void k_sh_given_records(const float4* __restrict__ normalMap, const float4* __restrict__ positionMap,
                                                               uint32_t n, float4* __restrict__ gbuf) {
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 nm = normalMap[i], pm = positionMap[i];
    gbuf[3 * size_t(i)] = make_float4(pm.x, pm.y, pm.z, 0.0f);
    gbuf[3 * size_t(i) + 1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(i));
    gbuf[3 * size_t(i) + 2] = make_float4(nm.x, nm.y, nm.z, 0.0f);
}

__global__ __launch_bounds__(LV_BLOCK) void k_sh_compact(const LvShCell* __restrict__ cells, uint32_t numCells, LvShCell* __restrict__ out,
                                                         uint32_t* __restrict__ outCount) {
    const uint32_t i = blockIdx.x * LV_BLOCK + threadIdx.x;
    const bool has = i < numCells && cells[i].key != 0ull;
    const unsigned long long m = __ballot(has);
    if (!m) return;
    uint32_t base = 0u;
    if (lv_lane() == 0u) base = atomicAdd(outCount, uint32_t(__popcll(m)));
    base = uint32_t(__shfl(base, 0, 64));
    if (has) out[base + uint32_t(__popcll(m & ((1ull << lv_lane()) - 1ull)))] = cells[i];
}

// the device buffers of map `which` (ctx->sh[which])
LvDeviceBuffer& lv_sh_cells(lv_ctx* ctx, const LvShState& M) { return &M == &ctx->sh[0] ? ctx->shMapCells : ctx->shGivenCells; }
LvDeviceBuffer& lv_sh_counters(lv_ctx* ctx, const LvShState& M) { return &M == &ctx->sh[0] ? ctx->shMapCounters : ctx->shGivenCounters; }

LvShParams lv_sh_params(const lv_ctx* ctx, const LvShState& M, uint32_t height, const float cam[3]) {
    LvShParams P;
    P.cam[0] = cam[0]; P.cam[1] = cam[1]; P.cam[2] = cam[2];
    P.tanSp = tanf(ctx->opt.shSp / float(height));
    P.sMin = powf(10.0f, float(ctx->opt.shSMinExp));
    P.sNd = ctx->opt.shSNd;
    P.numCells = M.numCells;
    return P;
}

// Allocates / re-keys the map for the options in force and queues k_sh_begin for a pass over w x h pixels.
int lv_sh_begin(lv_ctx* ctx, LvShState& M, uint32_t w, uint32_t h) {
    hipStream_t st = ctx->stream;
    int rc;
    const uint32_t numCells = ctx->opt.shNumCells;
    LvDeviceBuffer& cells = lv_sh_cells(ctx, M);
    LvDeviceBuffer& counters = lv_sh_counters(ctx, M);
    if (!cells.ptr || M.numCells != numCells) {
        // another size re-addresses every key: a new, empty map (this is a reset, not a counted clear)
        if (cells.ptr) { LV_HIP(ctx, hipStreamSynchronize(st)); lv_buf_free(cells); }
        if ((rc = lv_buf_reserve(ctx, cells, size_t(numCells) * sizeof(LvShCell)))) return rc;
        if ((rc = lv_buf_reserve(ctx, counters, sizeof(LvShCounters)))) return rc;
        M.numCells = numCells;
        LV_HIP(ctx, hipMemsetAsync(cells.ptr, 0, size_t(numCells) * sizeof(LvShCell), st));
        LV_HIP(ctx, hipMemsetAsync(counters.ptr, 0, sizeof(LvShCounters), st));
        M.clearPending = false;
        M.pixelsSinceClear = 0;
        M.sp = ctx->opt.shSp; M.sMinExp = ctx->opt.shSMinExp; M.sNd = ctx->opt.shSNd;
    }
    if (M.sp != ctx->opt.shSp || M.sMinExp != ctx->opt.shSMinExp || M.sNd != ctx->opt.shSNd) {
        M.clearPending = true;   // cells keyed with other parameters are never found again
        M.sp = ctx->opt.shSp; M.sMinExp = ctx->opt.shSMinExp; M.sNd = ctx->opt.shSNd;
    }
    const uint64_t pixels = uint64_t(w) * h;
    if (M.pixelsSinceClear + pixels >= (1ull << LV_SH_COUNT_BITS)) M.clearPending = true;
    const uint32_t force = M.clearPending ? 1u : 0u;
    if (force) M.pixelsSinceClear = 0;
    M.pixelsSinceClear += pixels;
    M.clearPending = false;
    const uint32_t grid = std::min(nblocks(numCells), uint32_t(ctx->numCUs) * 8u);
    k_sh_begin<<<grid, LV_BLOCK, 0, st>>>((LvShCell*)cells.ptr, numCells, (LvShCounters*)counters.ptr, force);
    return LV_OK;
}

// write + read of one denoise on the hits H (at most maxHits ordinals); readOut: w x h floats, cleared here
int lv_sh_passes(lv_ctx* ctx, LvShState& M, const LvShHits& H, uint64_t maxHits, uint32_t w, uint32_t h, const float cam[3],
                 const float* noisy, float* readOut) {
    hipStream_t st = ctx->stream;
    int rc;
    if (uint64_t(w) * h >= (1ull << LV_SH_COUNT_BITS)) return lv_fail(ctx, LV_E_CAPACITY, "Spatial Hashing: %u x %u pixels (fewer than 2^28)", w, h);
    if ((rc = lv_sh_begin(ctx, M, w, h))) return rc;
    const LvShParams P = lv_sh_params(ctx, M, h, cam);
    LvShCell* cells = (LvShCell*)lv_sh_cells(ctx, M).ptr;
    LvShCounters* c = (LvShCounters*)lv_sh_counters(ctx, M).ptr;
    LV_HIP(ctx, hipMemsetAsync(readOut, 0, size_t(w) * h * 4, st));
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_SH_WRITE, (k_sh_write<<<nblocks(maxHits), LV_BLOCK, 0, st>>>(H, P, noisy, cells, c)));
    LV_TIMED_LAUNCH(ctx, LV_KERNEL_SH_READ, (k_sh_read<<<nblocks(maxHits), LV_BLOCK, 0, st>>>(H, P, cells, readOut)));
    LV_HIP(ctx, hipGetLastError());
    return LV_OK;
}

} // namespace

// One denoise() of the renderer's map on the RTAO iteration just reduced into ctx->ao: the hits are the G-buffer's (ctx->aoGbuf, the
// group bases in tileBase), the result is the image *result points to afterwards.
int lv_sh_denoise_frame(lv_ctx* ctx, const float camPos[3], const uint32_t* tileBase, uint32_t numGroups, uint32_t tileW, uint32_t tileH,
                        uint32_t groupsX, uint32_t groupsPerTile, const uint32_t* hitCount, uint64_t maxPixels, const float** result) {
    hipStream_t st = ctx->stream;
    const uint32_t w = ctx->width, h = ctx->height;
    const size_t n = size_t(w) * h;
    int rc;
    for (LvDeviceBuffer* b : {&ctx->shNormal, &ctx->shPosition})
        if ((rc = lv_buf_reserve(ctx, *b, n * 16))) return rc;
    for (LvDeviceBuffer* b : {&ctx->shRead, &ctx->shPing, &ctx->shPong})
        if ((rc = lv_buf_reserve(ctx, *b, n * 4))) return rc;
    LvShHits H;
    H.gbuf = (const float4*)ctx->aoGbuf.ptr;
    H.tileBase = tileBase;
    H.numGroups = numGroups;
    H.layout.tileW = tileW; H.layout.tileH = tileH; H.layout.groupsX = groupsX; H.layout.groupsPerTile = groupsPerTile;
    H.count = hitCount;
    H.countImm = 0u;
    if ((rc = lv_sh_passes(ctx, ctx->sh[0], H, maxPixels, w, h, camPos, (const float*)ctx->ao.ptr, (float*)ctx->shRead.ptr))) return rc;
    LV_HIP(ctx, hipMemsetAsync(ctx->shNormal.ptr, 0, n * 16, st));
    LV_HIP(ctx, hipMemsetAsync(ctx->shPosition.ptr, 0, n * 16, st));
    k_sh_scatter_maps<<<nblocks(maxPixels), LV_BLOCK, 0, st>>>(H, (float4*)ctx->shNormal.ptr, (float4*)ctx->shPosition.ptr);
    LV_HIP(ctx, hipGetLastError());
    return lv_eaw_tail(ctx, w, h, (const float*)ctx->shRead.ptr, (const float4*)ctx->shNormal.ptr, (const float4*)ctx->shPosition.ptr,
                       (float*)ctx->shPing.ptr, (float*)ctx->shPong.ptr, result);
}

// lv_spatial_hashing_denoise_buffers: one denoise() on the caller's maps with the second map (ctx->sh[1]), which persists across calls.
// Every image of the call is a slice of ctx->shGiven (16-byte images first).
int lv_sh_denoise_given(lv_ctx* ctx, uint32_t w, uint32_t h, const float* noisy, const float* normalWorld, const float* positionWorld,
                        const float camPos[3], float* outRead, float* out) {
    const size_t n = size_t(w) * h;
    int rc;
    if ((rc = lv_buf_reserve(ctx, ctx->shGiven, n * (16 + 16 + 48 + 4 * 4)))) return rc;
    char* base = (char*)ctx->shGiven.ptr;
    size_t off = 0;
    auto slice = [&](size_t bytes) { char* p = base + off; off += bytes; return p; };
    float4* normalMap = (float4*)slice(n * 16);
    float4* positionMap = (float4*)slice(n * 16);
    float4* records = (float4*)slice(n * 48);
    float* raw = (float*)slice(n * 4);
    float* readImage = (float*)slice(n * 4);
    float* ping = (float*)slice(n * 4);
    float* pong = (float*)slice(n * 4);
    hipStream_t st = ctx->stream;
    LV_HIP(ctx, hipMemcpyAsync(normalMap, normalWorld, n * 16, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(positionMap, positionWorld, n * 16, hipMemcpyHostToDevice, st));
    LV_HIP(ctx, hipMemcpyAsync(raw, noisy, n * 4, hipMemcpyHostToDevice, st));
    k_sh_given_records<<<nblocks(n), LV_BLOCK, 0, st>>>(normalMap, positionMap, uint32_t(n), records);
    LvShHits H;
    H.gbuf = records;
    H.tileBase = nullptr;
    H.numGroups = 0u;
    H.layout.tileW = w; H.layout.tileH = h; H.layout.groupsX = 1u; H.layout.groupsPerTile = 1u;
    H.count = nullptr;
    H.countImm = uint32_t(n);
    if ((rc = lv_sh_passes(ctx, ctx->sh[1], H, n, w, h, camPos, raw, readImage))) return rc;
    const float* result = nullptr;
    if ((rc = lv_eaw_tail(ctx, w, h, readImage, normalMap, positionMap, ping, pong, &result))) return rc;
    if (outRead) LV_HIP(ctx, hipMemcpyAsync(outRead, readImage, n * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipMemcpyAsync(out, result, n * 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    return LV_OK;
}

// lv_spatial_hashing_reset: an empty map and zero statistics (a map that was never allocated is that already)
int lv_sh_reset(lv_ctx* ctx, int which) {
    LvShState& M = ctx->sh[which];
    M.clearPending = false;
    M.pixelsSinceClear = 0;
    if (!lv_sh_cells(ctx, M).ptr) return LV_OK;
    LV_HIP(ctx, hipMemsetAsync(lv_sh_cells(ctx, M).ptr, 0, size_t(M.numCells) * sizeof(LvShCell), ctx->stream));
    LV_HIP(ctx, hipMemsetAsync(lv_sh_counters(ctx, M).ptr, 0, sizeof(LvShCounters), ctx->stream));
    return LV_OK;
}

// the map leaves with the denoiser (lv_set_option): 16 B x spatial_hashing_num_cells are held only while it is selected
int lv_sh_release(lv_ctx* ctx, int which) {
    LvShState& M = ctx->sh[which];
    if (lv_sh_cells(ctx, M).ptr) {
        LV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        lv_buf_free(lv_sh_cells(ctx, M));
    }
    M.numCells = 0;
    M.clearPending = false;
    M.pixelsSinceClear = 0;
    return LV_OK;
}

int lv_sh_get_stats(lv_ctx* ctx, int which, uint64_t out[4]) {
    LvShState& M = ctx->sh[which];
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (!lv_sh_cells(ctx, M).ptr) return LV_OK;
    LvShCounters hc;
    LV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    LV_HIP(ctx, hipMemcpy(&hc, lv_sh_counters(ctx, M).ptr, sizeof hc, hipMemcpyDeviceToHost));
    out[0] = hc.occupied; out[1] = hc.stored; out[2] = hc.dropped; out[3] = hc.clears;
    return LV_OK;
}

int lv_sh_get_cells(lv_ctx* ctx, int which, uint64_t* keys, uint64_t* accumulators, uint64_t capacity, uint64_t* outCount) {
    LvShState& M = ctx->sh[which];
    *outCount = 0;
    if (!lv_sh_cells(ctx, M).ptr) return LV_OK;
    hipStream_t st = ctx->stream;
    int rc;
    // the compacted copy: at most numCells cells, then the count
    if ((rc = lv_buf_reserve(ctx, ctx->shCompact, size_t(M.numCells) * sizeof(LvShCell) + 16))) return rc;
    LvShCell* packed = (LvShCell*)ctx->shCompact.ptr;
    uint32_t* countDev = (uint32_t*)(packed + M.numCells);
    LV_HIP(ctx, hipMemsetAsync(countDev, 0, 4, st));
    k_sh_compact<<<nblocks(M.numCells), LV_BLOCK, 0, st>>>((const LvShCell*)lv_sh_cells(ctx, M).ptr, M.numCells, packed, countDev);
    uint32_t count = 0;
    LV_HIP(ctx, hipMemcpyAsync(&count, countDev, 4, hipMemcpyDeviceToHost, st));
    LV_HIP(ctx, hipStreamSynchronize(st));
    *outCount = count;
    if (!keys && !accumulators) return LV_OK;
    if (capacity < count) return lv_fail(ctx, LV_E_CAPACITY, "lv_spatial_hashing_get_cells: %u occupied cells, capacity %llu", count,
                                         (unsigned long long)capacity);
    std::vector<LvShCell> host(count);
    if (count) LV_HIP(ctx, hipMemcpy(host.data(), packed, size_t(count) * sizeof(LvShCell), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < count; i++) {
        if (keys) keys[i] = host[i].key;
        if (accumulators) accumulators[i] = host[i].acc;
    }
    return LV_OK;
}
