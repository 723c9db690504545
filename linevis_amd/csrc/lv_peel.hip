// lv_peel.hip -- the layer kernel of depth peeling (rendering mode 9).  The other kernels of modes 5 and 9 are lv_render.hip's; this
// one lives here because, as a kernel of that file, it changed the code the compiler generates for the existing kernels there that
// call lv_shade_prism and lv_prism_frag_pos, and those must compile to the instructions they had.
#include "lv_internal.h"
#include "lv_device.h"
#include "lv_trace.h"
#include "lv_prism.h"
#include "lv_peel.h"

namespace {

// One lane per viewport pixel, a wave = an 8 x 8 block of pixels.  Skips pixels that were not requested or are finished.
template <int SHADE, int FAST>
__global__ __launch_bounds__(LV_BLOCK, LV_PRISM_SHADE_MIN_WAVES) void k_peel_layer(const LvUniforms U, const LvSceneDev S,
                                                                   uint32_t* __restrict__ startOffset, LvPeelBuffers B) {
    __shared__ float s_prismRing[4 * LV_PRISM_MAX_SUBDIV];
    if (threadIdx.x < LV_PRISM_MAX_SUBDIV) {
        s_prismRing[threadIdx.x] = S.prism.c[threadIdx.x];
        s_prismRing[LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.s[threadIdx.x];
        s_prismRing[2 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.cp[threadIdx.x];
        s_prismRing[3 * LV_PRISM_MAX_SUBDIV + threadIdx.x] = S.prism.sn[threadIdx.x];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t blocksX = (U.width + 7u) / 8u;
    const uint32_t wave = blockIdx.x * (LV_BLOCK / LV_WAVE) + (threadIdx.x >> 6);
    const uint32_t px = (wave % blocksX) * 8u + (lane & 7u), py = (wave / blocksX) * 8u + (lane >> 3);
    if (px >= U.width || py >= U.height) return;
    const uint32_t addr = lv_ppll_addr(px, py, U.ppllPaddedW, U.ppllTileW, U.ppllTileH);
    if (startOffset[addr] != 0u) return;
    const unsigned long long won = B.slot[addr];
    if (won >= LV_PEEL_SLOT_EMPTY) {   // nothing left behind the last layer: no later pass can peel anything here
#if LV_PEEL_MASK_DONE
        startOffset[addr] = LV_PEEL_DONE;
#endif
        return;
    }
    const uint32_t key = uint32_t(won);
    const uint32_t leaf = S.segToLeaf[key >> 6], tt = key & 63u;
    const f3 o = mk3(U.camPos[0], U.camPos[1], U.camPos[2]);
    const float tLo = 0.0001f, tHi = __uint_as_float(__float_as_uint(1000.0f) + 1u);
    const float aoTexel = (U.useAmbientOcclusion && !U.aoPrebaked) ? S.ao[size_t(py) * U.width + px] : 1.0f;
    f3 oo, d;
    lv_primary_ray(U, px, py, 0.5f, 0.5f, oo, d);
    const LvRasterQuad rq = lv_make_raster_quad(U, px, py);
    bool kept;
    float depth;
    const f4 color = lv_shade_prism<SHADE, FAST>(S, U, s_prismRing, aoTexel, o, d, tLo, tHi, leaf, tt, rq, U.ppllRasterColour != 0u, depth, kept);
    B.accum[addr] = lv_peel_accumulate(B.accum[addr], color);
    B.prevZ[addr] = uint32_t(won >> 32);
    B.layers[addr] += 1u;
    B.slot[addr] = LV_PEEL_SLOT_EMPTY;
}

} // namespace

// SHADE / FAST as lv_frame_render selects the instances of the pooled fragment stage
void lv_peel_launch_layer(hipStream_t st, uint32_t grid, int shade, int fast, const LvUniforms& U, const LvSceneDev& S, uint32_t* startOffset,
                          const LvPeelBuffers& B) {
    if (fast == 2) k_peel_layer<LV_SHADE_PLAIN, 2><<<grid, LV_BLOCK, 0, st>>>(U, S, startOffset, B);
    else if (shade == LV_SHADE_BANDS) k_peel_layer<LV_SHADE_BANDS, 0><<<grid, LV_BLOCK, 0, st>>>(U, S, startOffset, B);
    else if (shade == LV_SHADE_HELICITY) k_peel_layer<LV_SHADE_HELICITY, 0><<<grid, LV_BLOCK, 0, st>>>(U, S, startOffset, B);
    else k_peel_layer<LV_SHADE_PLAIN, 0><<<grid, LV_BLOCK, 0, st>>>(U, S, startOffset, B);
}
