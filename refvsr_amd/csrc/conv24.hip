// 3x3 stride-1 convolutions with 24 output channels on fp16 HWC maps, everything a compile-time constant: the single-conv
// companion of resblock24.hip (same design: K order with immediate-offset B-fragment reads, hi + lo weights in three 16-row
// fragments with a half-wave fold, bias as the accumulators' initial value, one parameter blob per conv via LDS-DMA).
// Covers the conv shapes of the RefVSR_small family (mid_channels = 24) around the fused blocks:
//
//   NCG0 + NCG1 (16-byte channel groups of source 0 + source 1)
//   3 + 0   24 -> 24        ResList.conv_tail (RefVSR_/common.py:80-82), feat_fusion*.1 (RefVSR.py:53-62), ref_encoder*, conv_hr
//   2 + 0   16 -> 24        conf_fusion*.1 (RefVSR.py:47-52)
//   1 + 3   8 + 24 -> 24    ResidualBlocksWithInputConv.main.0 on cat([lr, feat]) (RefVSR.py:340-343)
//   3 + 3   24 + 24 -> 24   feat_fusion*.0 / feat_fusion2_1 / fusion_UP on cat([a, b]) (RefVSR.py:53-62,87)
//
// out = post( act(conv + bias) * mul + res ), the epilogue of refvsr_conv_mfma's fp16 HWC mode.  The generic kernel stays
// for every other shape (strides, 5x5 / 7x7, pixel shuffle, planar outputs, other channel counts).
//
// COUT = 32 (AlignedConv2d's 32-channel convs, RefVSR_/alignment.py:18-24): four fragments per K-step ([hi | lo] of output channels
// 0-15, 16-31), inputs 32 (NCG 4) and 8 (NCG 1: the RGB stem; K plan: the three taps of a window row + a zero block per step).
//
// COUT = 48 (the mid_channels = 48 family, configs/config_RefVSR_{L1,MFID,MFID_8K}.py: 30 ResidualBlockNoBN per branch, two
// convs each): six fragments per K-step ([hi | lo] of output channels 0-15, 16-31, 32-47; no fold), 48 -> 48 with the 84 KB
// weight set resident next to a 16 x 32-pixel tile (18 x 34 staged pixels, 68 KB) walked by SIXTEEN waves -- one workgroup per
// CU, four waves per SIMD, 255 tiles for the 270 x 480 map of the 256-CU chip -- and 16 -> 48 on the 8 x 32 tile.
//
// SHUF = 24 | 48 (PixelShufflePack.upsample_conv + F.pixel_shuffle, mmedit upsample.py:36-51; RefVSR.py:89-90,138): the
// C -> 4 C conv as groups of 48 output rows on the COUT = 48 kernel, blockIdx.y = group z, rows ordered sub-pixel-major so that
// a lane's four accumulator rows are four consecutive channels of ONE sub-pixel: C = 24: group z = output row parity dy, rows
// [dx = 0: channels 0-23][dx = 1: channels 0-23]; C = 48: group z = sub-pixel 2 dy + dx, rows = channels 0-47.  The epilogue
// stores straight into the [2h][2w][C] map (bias + optional leaky activation; no multiplier / residual on this layer).
//
// LDS: [fragments: S K-steps x 3 x 1 KiB][bias: 32 floats][x tile: 10 x 34 pixels x PS slots of 16 bytes, PS = NCG | 1 (odd
// pixel stride: bank-conflict-free B reads with the pixel permutation of common.h)].  K plans (c24_kblock): the K-blocks of
// one window row are the slots u = tx * PS + cg; a K-step takes four of them whose offsets are (step immediate) + (one of
// <= 4 per-lane patterns), the two blocks a ds_read_b128 lane group mixes having slot offsets of equal parity:
//   NCG 3: rows of 9 consecutive slots -> 2 steps of {0,2,1,3} + 4a per row, then u = 8 of the three rows   (7 steps)
//   NCG 4: one step per tap, cg = {0,2,1,3}                                                                  (9 steps)
//   NCG 2: u = {0,4,1,3} per row, then u = 6 | 7 of rows 0,1, then of row 2                                  (5 steps)
//   NCG 6: one step per tap with cg = {0,2,1,3}; cg 4,5 of taps (tx 0, tx 1) per row; of tx 2 for rows 0,1; for row 2   (14 steps)
#include "common.h"
#include "fixed_plan.h"

struct C24Args {
    const unsigned char* src0; const unsigned char* src1; unsigned char* out;
    const unsigned char* blob; const unsigned char* mul; const unsigned char* res;
    int h, w, tiles_x, n_tiles, grid;
    float act_slope, post_slope;
    // CONF variants (refvsr_conf_alpha): the 16-channel input map is not read, it is COMPUTED while the tile is staged
    const float* conf_a; const float* conf_b;    // the two planar fp32 confidence maps [ch][cw]
    const float* cw0; const float* cb0;          // first conv of the pair: fp32 weights [16][2][3][3], bias [16]
    float* conf_max;                             // optional by-product max(conf_a, conf_b) [ch][cw] (CONF = 1)
    int ch, cw;                                  // size of the confidence maps (CONF = 2: half the conv's grid)
    float slope0;
    // COUT = 3 (refvsr_conv_last): `out` is planar fp32 [3][h][w]; base_lr: the LR centre frame, planar fp32 [3][bh][bw], whose
    // bicubic up-sampling (clamped to [0, 1]) is added before the final clamp
    const float* base_lr; int bh, bw; float base_step;
    int out_fmt;                                 // COUT = 3: REFVSR_RESULT_* of `out` (| REFVSR_RESULT_HWC)
    // Multi-map launches (refvsr_*_batch, ABI 11): batch > 1 maps of one geometry share the launch and the weight fill; flat tile
    // index t = b * tpm + (tile of map b); map b's operands come from the tables (entry 0 == the scalar fields above, which stay
    // the "operand present" flags).  Not for the HALF variant.
    int batch, tpm;
    const unsigned char* bsrc0[REFVSR_MAX_MAPS]; const unsigned char* bsrc1[REFVSR_MAX_MAPS]; unsigned char* bout[REFVSR_MAX_MAPS];
    const unsigned char* bmul[REFVSR_MAX_MAPS]; const unsigned char* bres[REFVSR_MAX_MAPS];
    const float* bconf_a[REFVSR_MAX_MAPS]; const float* bconf_b[REFVSR_MAX_MAPS]; float* bconf_max[REFVSR_MAX_MAPS];
};

// COUT = 24 | 48 output channels; TH = 8 | 16 tile rows; NWV waves walk the TH x 32 tile, T = 2 TH / NWV pixel groups per wave;
// WPS = waves per SIMD the kernel is built for (register budget).
// CONF = 1 | 2 (16 -> COUT convs of the confidence fusions, RefVSR.py:47-52,130,141-142,107-109): the kernel's 16-channel
// input  a = lrelu(conv3x3_{2->16}(cat[conf_a, conf_b]))  -- for CONF = 2 of the pair up-sampled x2 (bicubic, clamped to [0, 1]) --
// is evaluated per staged pixel from the two fp32 confidence maps instead of being read: torch.cat, [F.interpolate,] the
// 2 -> 16 conv (refvsr_conv_direct_f32's fp32 FMA order, fp16 rounding) and for CONF = 1 the torch.max of the two maps
// (RefVSR.py:147) leave the launch list; results are bit-identical to the separate launches.
// HALF = 1 (48 + 48 -> 48, the two-source convs of the mid_channels = 48 models: feat_fusion*.0 / feat_fusion2_1 / fusion_UP on
// cat([a, b]), RefVSR.py:53-62,87): one conv's hi + lo weights are 166 KB -- no resident form.  The OUTPUT channels are split
// instead: blockIdx.y = z computes channels 24 z .. 24 z + 23 with the 24-row fragment trick (81 KB of weights per half, NCG = 12
// plan, 70 KB tile: one sixteen-wave workgroup per CU) and stores them into the 48-channel maps at byte offset 48 z.
// MM = 1 (ABI 11): multi-map launch -- p.batch maps behind one weight fill (the batched entry points; the single-map instantiations
// are untouched by it).
// WF: weight format (fixed_plan.h:c24_nf); WF = 1 issues the hi MFMAs of WF = 0 in the same order on the same accumulators and drops the lo ones
// (which add exact zeros for fp16-representable weights): bit-identical results on such weights.
template <int COUT, int NCG0, int NCG1, int NWV, int TH, int WPS, int SHUF = 0, int CONF = 0, int HALF = 0, int MM = 0, int WF = 0>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(WPS, WPS))) void conv24_kernel(C24Args p) {
    static_assert(WF == 0 || COUT != 3, "output head: one fragment in either format");
    static_assert(HALF == 0 || (COUT == 24 && SHUF == 0 && CONF == 0), "channel-half variant: 24 computed channels per workgroup");
    static_assert(MM == 0 || (HALF == 0 && COUT != 3), "multi-map variant");
    static_assert(SHUF == 0 || (COUT == 48 && (SHUF == 24 || SHUF == 48) && NCG0 * 8 == SHUF && NCG1 == 0), "pixel-shuffle variant");
    static_assert(CONF == 0 || (NCG0 == 2 && NCG1 == 0 && SHUF == 0), "confidence variant: 16-channel single source");
    constexpr int NCG = NCG0 + NCG1, PS = NCG | 1, PXB = PS * 16, ROWB = C24_XW * PXB;
    constexpr int S = c24_steps(NCG), NPAT = c24_npat(NCG);
    constexpr int NF = c24_nf(COUT, WF);                             // fragments per K-step
    constexpr int NM = COUT == 24 ? 2 : COUT == 3 ? 1 : COUT / 16;  // accumulator tiles per pixel group
    constexpr int BIASB = COUT == 48 ? 256 : 128;
    constexpr int WB = S * NF * 1024, BIAS = WB, XT = WB + BIASB;
    constexpr int NT = NWV * 64, T = 2 * TH / NWV;
    constexpr int C24_TH = TH, C24_XH = TH + 2, C24_NPX = C24_XH * C24_XW;
    constexpr int NCH = C24_NPX * NCG, KCH = (NCH + NT - 1) / NT;
    constexpr int PIXB0 = NCG0 * 16, PIXB1 = NCG1 * 16;
    constexpr int OPX = HALF ? 96 : COUT * 2;                       // bytes per pixel of the out / mul / res maps
    static_assert((COUT == 3 || COUT == 24 || COUT == 32 || COUT == 48) && S > 0 && T >= 1 && T * NWV == 2 * TH, "unsupported shape");
    static_assert(COUT != 3 || (NCG1 == 0 && SHUF == 0 && CONF == 0), "output head: single source");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    asm volatile("" :: "s"(p.src0), "s"(p.src1), "s"(p.out), "s"(p.blob), "s"(p.mul), "s"(p.res), "s"(p.h), "s"(p.w), "s"(p.tiles_x),
                 "s"(p.n_tiles), "s"(p.grid), "s"(p.act_slope), "s"(p.post_slope));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- weights + bias: global -> LDS (1 KiB per wave instruction), issued first
    {
        constexpr int NPC = WB / 1024;                               // full pieces; the 128-byte bias tail: 8 lanes
        const unsigned char* g = p.blob + ((SHUF || HALF) ? (int)blockIdx.y * (WB + BIASB) : 0) + lane * 16;   // SHUF / HALF: one blob per row group
#pragma unroll
        for (int j = 0; j < (NPC + NWV - 1) / NWV; ++j) {
            const int c = wave + j * NWV;
            if (c < NPC)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + c * 1024),
                                                 (__attribute__((address_space(3))) void*)(smem + c * 1024), 16, 0, 0);
        }
        if (wave == NPC % NWV && lane < BIASB / 16)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + NPC * 1024),
                                             (__attribute__((address_space(3))) void*)(smem + NPC * 1024), 16, 0, 0);
    }

    if constexpr (HALF != 0) {                                       // this workgroup's 24 channels inside the 48-channel maps
        const int zoff = (int)blockIdx.y * 48;
        p.out += zoff;
        if (p.mul) p.mul += zoff;
        if (p.res) p.res += zoff;
    }
    // ---- x-tile chunks of this thread: i = tid + k NT = pixel * NCG + cg; global offset relative to the tile origin of its
    //      source, LDS offset, source flag -- computed once
    const int rowp = p.w;
    unsigned xg[KCH], xl[KCH];
    unsigned xs1 = 0;                                                // bit k: chunk k comes from source 1
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const int i = min(tid + k * NT, NCH - 1);
        const int px = i / NCG, cg = i - px * NCG;
        const int r = px / C24_XW, c = px - r * C24_XW;
        const bool s1 = cg >= NCG0;
        xg[k] = (unsigned)((r * rowp + c) * (s1 ? PIXB1 : PIXB0) + (s1 ? cg - NCG0 : cg) * 16);
        xl[k] = (unsigned)(XT + px * PXB + cg * 16);
        xs1 |= s1 ? (1u << k) : 0u;
    }
    uint4 xv[KCH];
    auto x_fetch = [&](const int tf) {
        int t = tf;
        const unsigned char* s0p = p.src0;
        const unsigned char* s1p = p.src1;
        if constexpr (MM != 0) {                                     // flat tile index -> (map, tile of the map); uniform
            const int bm = (int)((unsigned)tf / (unsigned)p.tpm);
            t = tf - bm * p.tpm;
            s0p = p.bsrc0[bm];
            if constexpr (NCG1 != 0) s1p = p.bsrc1[bm];
        }
        const int tyi = t / p.tiles_x;
        const int ty0 = tyi * C24_TH, tx0 = (t - tyi * p.tiles_x) * C24_TW;
        const bool interior = ty0 >= 1 && ty0 + C24_TH + 1 <= p.h && tx0 >= 1 && tx0 + C24_TW + 1 <= p.w;
        const long long org = (long long)(ty0 - 1) * p.w + (tx0 - 1);          // origin pixel (may lie outside the frame)
        const unsigned char* b0 = s0p + org * PIXB0;
        const unsigned char* b1 = NCG1 ? s1p + org * PIXB1 : b0;
        if (interior) {
#pragma unroll
            for (int k = 0; k < KCH; ++k)
                xv[k] = *reinterpret_cast<const uint4*>((NCG1 && ((xs1 >> k) & 1) ? b1 : b0) + xg[k]);
        } else {
            int tide = tid;                                           // opaque: keeps this path's index math inside the branch
            asm volatile("" : "+v"(tide));
#pragma unroll
            for (int k = 0; k < KCH; ++k) {
                const int i = min(tide + k * NT, NCH - 1);
                const int px = i / NCG, cg = i - px * NCG;
                const int r = px / C24_XW, c = px - r * C24_XW;
                const int iy = ty0 - 1 + r, ix = tx0 - 1 + c;
                const bool ok = (unsigned)iy < (unsigned)p.h && (unsigned)ix < (unsigned)p.w;
                const bool s1 = cg >= NCG0;
                const unsigned pix = (unsigned)(min(max(iy, 0), p.h - 1) * p.w + min(max(ix, 0), p.w - 1));
                const unsigned char* g = s1 ? s1p + pix * PIXB1 + (cg - NCG0) * 16 : s0p + pix * PIXB0 + cg * 16;
                uint4 v = *reinterpret_cast<const uint4*>(g);        // clamped address, masked value (32-bit offsets: host check)
                const unsigned keep = ok ? 0xffffffffu : 0u;
                v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
                xv[k] = v;
            }
        }
    };
    auto x_park = [&]() {
#pragma unroll
        for (int k = 0; k < KCH; ++k)
            if (k * NT + NT <= NCH || tid + k * NT < NCH) *reinterpret_cast<uint4*>(smem + xl[k]) = xv[k];
    };
    // ---- CONF: LDS behind the x tile: [pair tile: 2 x (TH + 4) x 36 floats][first conv: 18 taps x 16 outputs][its bias: 16]
    constexpr int PTH = TH + 4, PTW = C24_XW + 2;
    constexpr int PT = XT + C24_NPX * PXB, CW0 = PT + 2 * PTH * PTW * 4, CB0 = CW0 + 18 * 16 * 4;
    if constexpr (CONF != 0) {
        float* wl0 = reinterpret_cast<float*>(smem + CW0);            // [tap = ci * 9 + ky * 3 + kx][co]: 64-byte rows, co fastest
        for (int i = tid; i < 18 * 16; i += NT) {
            const int co = i & 15, tap = i >> 4;
            wl0[i] = p.cw0[(co * 2 + tap / 9) * 9 + tap % 9];
        }
        if (tid < 16) reinterpret_cast<float*>(smem + CB0)[tid] = p.cb0[tid];
    }
    // the whole x tile of tile t, computed: stage 1 = the (TH + 4) x 36 window of the pair (zero outside the frame = the first
    // conv's padding; CONF = 2: clamp01(bicubic x2) of the half-size maps), stage 2 = lrelu(conv 2 -> 16) per staged pixel
    // (zero outside the frame = the second conv's padding).  Called by all threads; contains one barrier.
    auto conf_stage = [&](const int tf) {
        int t = tf;
        const float* cap = p.conf_a;
        const float* cbp = p.conf_b;
        float* cmp_ = p.conf_max;
        if constexpr (MM != 0) {
            const int bm = (int)((unsigned)tf / (unsigned)p.tpm);
            t = tf - bm * p.tpm;
            cap = p.bconf_a[bm]; cbp = p.bconf_b[bm];
            if (p.conf_max) cmp_ = p.bconf_max[bm];
        }
        const int tyi = t / p.tiles_x;
        const int ty0 = tyi * C24_TH, tx0 = (t - tyi * p.tiles_x) * C24_TW;
        float* pt = reinterpret_cast<float*>(smem + PT);
        for (int i = tid; i < 2 * PTH * PTW; i += NT) {
            const int c = i / (PTH * PTW), rem = i - c * (PTH * PTW);
            const int r = rem / PTW, cc = rem - r * PTW;
            const int y = ty0 - 2 + r, x = tx0 - 2 + cc;
            float v = 0.0f;
            if ((unsigned)y < (unsigned)p.h && (unsigned)x < (unsigned)p.w) {
                const float* src = c ? cbp : cap;
                if constexpr (CONF == 1) v = src[(size_t)y * p.cw + x];
                else v = fminf(fmaxf(rv_bicubic_at(src, p.ch, p.cw, y, x, 0.5f, 0.5f), 0.0f), 1.0f);
            }
            pt[i] = v;
        }
        __syncthreads();
        const float* wl0 = reinterpret_cast<const float*>(smem + CW0);
        const float* bl0 = reinterpret_cast<const float*>(smem + CB0);
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const int i = tid + k * NT;
            if (i < NCH) {
                const int px = i >> 1, cg = i & 1;
                const int r = px / C24_XW, c = px - r * C24_XW;
                const int iy = ty0 - 1 + r, ix = tx0 - 1 + c;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if ((unsigned)iy < (unsigned)p.h && (unsigned)ix < (unsigned)p.w) {
                    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                            for (int kx = 0; kx < 3; ++kx) {             // conv_direct.hip's order: ci, ky, kx; acc = fma(x, w, acc)
                                const float xv = pt[ci * (PTH * PTW) + (r + ky) * PTW + (c + kx)];
                                const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl0 + (ci * 9 + ky * 3 + kx) * 16 + cg * 8);
                                const f32x4 w1 = *reinterpret_cast<const f32x4*>(wl0 + (ci * 9 + ky * 3 + kx) * 16 + cg * 8 + 4);
                                acc[0] = fmaf(xv, w0[0], acc[0]); acc[1] = fmaf(xv, w0[1], acc[1]);
                                acc[2] = fmaf(xv, w0[2], acc[2]); acc[3] = fmaf(xv, w0[3], acc[3]);
                                acc[4] = fmaf(xv, w1[0], acc[4]); acc[5] = fmaf(xv, w1[1], acc[5]);
                                acc[6] = fmaf(xv, w1[2], acc[6]); acc[7] = fmaf(xv, w1[3], acc[7]);
                            }
                    union { f16x8 h; uint4 u; } o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) o.h[j] = (f16)rv_lrelu(acc[j] + bl0[cg * 8 + j], p.slope0);
                    v = o.u;
                }
                *reinterpret_cast<uint4*>(smem + XT + px * PXB + cg * 16) = v;
            }
        }
        if constexpr (CONF == 1) {
            if (p.conf_max) {                                          // RefVSR.py:147 for the pixels this tile owns
                for (int i = tid; i < C24_TH * C24_TW; i += NT) {
                    const int r = i / C24_TW, c = i - r * C24_TW;
                    const int y = ty0 + r, x = tx0 + c;
                    if (y < p.h && x < p.w)
                        cmp_[(size_t)y * p.w + x] = fmaxf(pt[(r + 2) * PTW + c + 2], pt[PTH * PTW + (r + 2) * PTW + c + 2]);
                }
            }
        }
    };
    int tl, k_hi;
    rv_tile_range(p.n_tiles, p.grid, tl, k_hi);
    if constexpr (CONF == 0) { if (tl < k_hi) x_fetch(tl); }
    __builtin_amdgcn_sched_barrier(0);                               // weights and first tile in flight before the rest of the set-up

    // ---- per-lane constants
    const int q = lane >> 4;
    const int lp = rv_pix16(lane & 15);
    const int la = lane * 16;
    // pixel group t of this wave = group wave * T + t of the tile: output row RW(t), left | right half CG(t) (T odd: NWV = 2 TH)
    const int g0w = wave * T;
#define RW(t) ((g0w + (t)) >> 1)
#define CG(t) ((g0w + (t)) & 1)
    auto sel4 = [&](const int v0, const int v1, const int v2, const int v3) { return q == 0 ? v0 : q == 1 ? v1 : q == 2 ? v2 : v3; };
    int pb[T];                                                       // window origin of each output group + this lane's pattern-0 offset
#pragma unroll
    for (int t = 0; t < T; ++t)
        pb[t] = XT + RW(t) * ROWB + (CG(t) * 16 + lp) * PXB +
                sel4(c24_off(NCG, 0, 0), c24_off(NCG, 0, 1), c24_off(NCG, 0, 2), c24_off(NCG, 0, 3)) - c24_off(NCG, 0, 0);
    int pd[NPAT];                                                    // pattern p relative to pattern 0, per lane
#pragma unroll
    for (int pp = 0; pp < NPAT; ++pp) {
        const int s = c24_pat_step(NCG, pp);
        pd[pp] = (sel4(c24_off(NCG, s, 0), c24_off(NCG, s, 1), c24_off(NCG, s, 2), c24_off(NCG, s, 3)) - c24_off(NCG, s, 0)) -
                 (sel4(c24_off(NCG, 0, 0), c24_off(NCG, 0, 1), c24_off(NCG, 0, 2), c24_off(NCG, 0, 3)) - c24_off(NCG, 0, 0));
    }
    const int rowb_o = p.w * OPX;
    const unsigned oo = (unsigned)(lp * OPX + q * 8);                // this lane's channels 4q.. of its pixel, relative to the group's origin

    if constexpr (CONF == 0) { if (tl < k_hi) x_park(); }
    __syncthreads();                                                 // weights, bias, first tile (CONF: first-conv weights)

    for (; tl < k_hi; ++tl) {
        const bool has_next = tl + 1 < k_hi;
        if constexpr (CONF != 0) {                                   // the tile is computed, not prefetched: staged at the top
            conf_stage(tl);
            __syncthreads();
        }
        int tm = tl;
        unsigned char* outp = p.out;
        const unsigned char* mulp = p.mul;
        const unsigned char* resp = p.res;
        if constexpr (MM != 0) {
            const int bm = (int)((unsigned)tl / (unsigned)p.tpm);
            tm = tl - bm * p.tpm;
            outp = p.bout[bm];
            if (p.mul) mulp = p.bmul[bm];
            if (p.res) resp = p.bres[bm];
        }
        const int tyi = tm / p.tiles_x;
        const int ty0 = tyi * C24_TH, tx0 = (tm - tyi * p.tiles_x) * C24_TW;
        const bool interior = ty0 >= 1 && ty0 + C24_TH + 1 <= p.h && tx0 >= 1 && tx0 + C24_TW + 1 <= p.w;
        const long long oorg = ((long long)ty0 * p.w + tx0) * OPX;
        // epilogue operands of this tile, in flight during the K loop.  Accumulator tile m of a pixel group holds channels
        // 16 m + 4 q .. (COUT = 24: tile 1 = channels 16 + 4 q for q < 2, see resblock24.hip)
        f16x4 mv[NM][T], rv[NM][T];
        bool okt[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            okt[t] = true;
            if (!interior) {
                int lpe = lp;
                asm volatile("" : "+v"(lpe));
                okt[t] = ty0 + RW(t) < p.h && tx0 + CG(t) * 16 + lpe < p.w;
            }
            const unsigned eo = (unsigned)(RW(t) * rowb_o) + oo + CG(t) * 16 * OPX;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                mv[m][t] = rv[m][t] = (f16x4){(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
                const bool lane_ok = okt[t] && (COUT != 24 || m == 0 || q < 2);
                if constexpr (COUT == 24) {                          // (COUT = 48: fetched in the epilogue -- register budget)
                    if (p.mul && lane_ok) mv[m][t] = *reinterpret_cast<const f16x4*>(mulp + oorg + eo + 32 * m);
                    if (p.res && lane_ok) rv[m][t] = *reinterpret_cast<const f16x4*>(resp + oorg + eo + 32 * m);
                }
                (void)lane_ok;
            }
        }
        if constexpr (CONF == 0) { if (has_next) x_fetch(tl + 1); }  // next tile: in flight during the K loop

        // ---------------- K loop: acc = bias + conv(x) on the TH x 32 tile ---------------------------------------------------
        f32x4 acc[NM][T];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(smem + BIAS + m * 64 + q * 16);   // channels 16 m + 4 q .. (pads: zeros)
#pragma unroll
            for (int t = 0; t < T; ++t) acc[m][t] = bv;
        }
        {
            uint4 fa[2][NF], fb[2][T];
            auto load = [&](auto sc, uint4 (&af)[NF], uint4 (&bf)[T]) {
                constexpr int s = decltype(sc)::value;
                constexpr int pp = c24_pat(NCG, s);
                constexpr int imm = c24_off(NCG, s, 0);
#pragma unroll
                for (int f = 0; f < NF; ++f) af[f] = *reinterpret_cast<const uint4*>(smem + (s * NF + f) * 1024 + la);
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    if constexpr (pp == 0) bf[t] = *reinterpret_cast<const uint4*>(smem + pb[t] + imm);
                    else bf[t] = *reinterpret_cast<const uint4*>(smem + pb[t] + pd[pp] + imm);
                }
            };
            auto mfma = [&](const uint4 (&af)[NF], const uint4 (&bf)[T]) {
                if constexpr (WF == 1) {                             // [rows 16 m ..] per accumulator tile
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const f16x8 av = *reinterpret_cast<const f16x8*>(&af[m]);
#pragma unroll
                        for (int t = 0; t < T; ++t)
                            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, *reinterpret_cast<const f16x8*>(&bf[t]), acc[m][t], 0, 0, 0);
                    }
                } else if constexpr (COUT == 24) {                   // [hi 0-15] [lo 0-15] [hi 16-23 | lo 16-23]
                    const f16x8 a_hi = *reinterpret_cast<const f16x8*>(&af[0]);
                    const f16x8 a_lo = *reinterpret_cast<const f16x8*>(&af[1]);
                    const f16x8 a_mx = *reinterpret_cast<const f16x8*>(&af[2]);
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, *reinterpret_cast<const f16x8*>(&bf[t]), acc[0][t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_mx, *reinterpret_cast<const f16x8*>(&bf[t]), acc[1][t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, *reinterpret_cast<const f16x8*>(&bf[t]), acc[0][t], 0, 0, 0);
                } else if constexpr (COUT == 3) {                    // ONE fragment: rows 0-2 = hi, rows 8-10 = lo (folded in the epilogue)
                    const f16x8 a_w = *reinterpret_cast<const f16x8*>(&af[0]);
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_w, *reinterpret_cast<const f16x8*>(&bf[t]), acc[0][t], 0, 0, 0);
                } else {                                             // [hi | lo] of channels 0-15, 16-31, 32-47: all hi, then all lo
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int m = 0; m < NM; ++m) {
                            const f16x8 av = *reinterpret_cast<const f16x8*>(&af[2 * m + h]);
#pragma unroll
                            for (int t = 0; t < T; ++t)
                                acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, *reinterpret_cast<const f16x8*>(&bf[t]), acc[m][t], 0, 0, 0);
                        }
                }
            };
            if constexpr (NF <= 4) {
                // two fragment sets: the reads of step s + 1 are issued above the MFMAs of step s (WF = 1: every shape, COUT = 48 too)
                load(std::integral_constant<int, 0>{}, fa[0], fb[0]);
                rv_static_for([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    if constexpr (s + 1 < S) load(std::integral_constant<int, s + 1>{}, fa[(s + 1) & 1], fb[(s + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma(fa[s & 1], fb[s & 1]);
                }, std::make_integer_sequence<int, S>{});
            } else {
                // ONE fragment set (six weight fragments: a second set does not fit 128 VGPRs): the reads of step s + 1 are issued
                // right behind the 6 T MFMAs of step s -- those have latched their operands by then and occupy the matrix pipe for
                // 96 T cycles, longer than the reads take
                load(std::integral_constant<int, 0>{}, fa[0], fb[0]);
                rv_static_for([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    __builtin_amdgcn_sched_barrier(0);
                    mfma(fa[0], fb[0]);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (s + 1 < S) load(std::integral_constant<int, s + 1>{}, fa[0], fb[0]);
                }, std::make_integer_sequence<int, S>{});
            }
        }
        if (has_next) {
            __syncthreads();                                         // every wave is done reading the x tile
            if constexpr (CONF == 0) x_park();
        }
        if constexpr (COUT == 3) {
            // ---------------- output head (RefVSR.py:118,288,297): clamp( conv + bias + clamp01(bicubic(lr_centre)), 0, 1 ) -> planar fp32.
            // After the fold lane (0, n) holds the three channel sums of pixel n of the group; lane (q, n), q < 3, takes channel q
            // (ds_bpermute), evaluates ITS channel's bicubic sample (rv_bicubic_at: resize_kernel<BICUBIC>'s FMA chains) and stores one
            // value: 48 lanes x 4 bytes = three 64-byte row segments per group (planar), or with REFVSR_RESULT_HWC one 192-byte segment
            // [16 pixels][3], lane (q, n) on element 3 lp + q (rv_result_index: the layout moves the address, never the value; a variant
            // with lane e on element e -- one contiguous run per wave -- scatters the lanes' bicubic taps over the three base planes
            // and measured 2 - 2.7 x slower, profiles/result_layout_timing.txt).  Resource usage with the layout select
            // (-Rpass-analysis=kernel-resource-usage): C = 24 88 VGPRs (78 before it), C = 48 104 (94); no scratch, 4 waves per SIMD as before
            const size_t plane_b = (size_t)p.bh * p.bw;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const f32x4 y = acc[0][t];
                const float s0 = rv_fold1(y[0]), s1 = rv_fold1(y[1]), s2 = rv_fold1(y[2]);
                const int srcl = lane & 15;
                const float v0 = __shfl(s0, srcl), v1 = __shfl(s1, srcl), v2 = __shfl(s2, srcl);
                const float v = q == 0 ? v0 : q == 1 ? v1 : v2;
                int lpe = lp;
                if (!interior) asm volatile("" : "+v"(lpe));
                const int oy = ty0 + RW(t), ox = tx0 + CG(t) * 16 + lpe;
                if (q < 3 && oy < p.h && ox < p.w) {
                    const float b = fminf(fmaxf(rv_bicubic_at(p.base_lr + q * plane_b, p.bh, p.bw, oy, ox, p.base_step, p.base_step), 0.0f), 1.0f);
                    rv_store_result(outp, rv_result_index(p.out_fmt, q, oy, ox, p.h, p.w), fminf(fmaxf(v + b, 0.0f), 1.0f), p.out_fmt);
                }
            }
        } else if constexpr (SHUF != 0) {
            // ---------------- pixel-shuffle epilogue: rows 16 m + 4 q .. of group z -> channels ch0 .. of sub-pixel (dy, dx) -------
            const int z = (int)blockIdx.y;
            const unsigned w2 = 2u * (unsigned)p.w;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                int lpe = lp;
                if (!interior) asm volatile("" : "+v"(lpe));
                const unsigned oy = (unsigned)(ty0 + RW(t)), ox = (unsigned)(tx0 + CG(t) * 16 + lpe);
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    const int r0 = 16 * m + 4 * q;
                    const int dx = SHUF == 24 ? (r0 >= 24 ? 1 : 0) : (z & 1);
                    const int dy = SHUF == 24 ? z : (z >> 1);
                    const int ch0 = SHUF == 24 ? r0 - 24 * dx : r0;
                    f32x4 y = acc[m][t];
                    if (p.act_slope != 1.0f) {                       // (the activation commutes with the shuffle: RefVSR.py:116)
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * p.act_slope);
                    }
                    const f16x4 o = {(f16)y[0], (f16)y[1], (f16)y[2], (f16)y[3]};
                    if (okt[t])
                        *reinterpret_cast<f16x4*>(outp + ((2u * oy + dy) * w2 + 2u * ox + dx) * (unsigned)(SHUF * 2) + ch0 * 2) = o;
                }
            }
        } else
        // ---------------- epilogue: out = post(act(acc) * mul + res) ----------------------------------------------------------
        {
            unsigned char* ob = outp + oorg;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                unsigned char* d = ob + (unsigned)(RW(t) * rowb_o) + oo + CG(t) * 16 * OPX;
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    f32x4 y = acc[m][t];
                    if constexpr (COUT == 24) {
                        if (WF == 0 && m == 1) y = (f32x4){rv_fold1(y[0]), rv_fold1(y[1]), rv_fold1(y[2]), rv_fold1(y[3])};
                    } else {
                        const unsigned eo = (unsigned)(RW(t) * rowb_o) + oo + CG(t) * 16 * OPX;
                        if (p.mul && okt[t]) mv[m][t] = *reinterpret_cast<const f16x4*>(mulp + oorg + eo + 32 * m);
                        if (p.res && okt[t]) rv[m][t] = *reinterpret_cast<const f16x4*>(resp + oorg + eo + 32 * m);
                    }
                    if (p.act_slope != 1.0f) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * p.act_slope);
                    }
                    if (p.mul) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] *= (float)mv[m][t][i];
                    }
                    if (p.res) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] += (float)rv[m][t][i];
                    }
                    if (p.post_slope != 1.0f) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[i] = fmaxf(y[i], y[i] * p.post_slope);
                    }
                    const f16x4 o = {(f16)y[0], (f16)y[1], (f16)y[2], (f16)y[3]};
                    if (okt[t] && (COUT != 24 || m == 0 || q < 2)) *reinterpret_cast<f16x4*>(d + 32 * m) = o;
                }
            }
        }
        if constexpr (CONF == 0) { if (has_next) __syncthreads(); }  // next x tile visible
    }
#undef RW
#undef CG
}

template <int COUT, int NCG0, int NCG1, int NWV, int TH, int WPS, int SHUF, int CONF, int HALF, int MM, int WF>
static int launch_c24(C24Args& a, const C24Plan& p, hipStream_t st) {
    constexpr int NZ = c24_nz(SHUF, HALF), LDS = c24_lds(COUT, NCG0 + NCG1, TH, CONF, WF);
    static_assert(LDS <= 160 * 1024, "LDS budget");
    static RvLaunchCap lc = {};
    int cap;
    if (int rc = rv_launch_cap(lc, &conv24_kernel<COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF>, NWV * 64, LDS, LDS, st, &cap, NZ)) return rc;
    a.tiles_x = p.tiles_x; a.tpm = p.tpm; a.n_tiles = p.n_tiles;
    a.grid = a.n_tiles < cap ? a.n_tiles : cap;
    hipLaunchKernelGGL((conv24_kernel<COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF>), dim3(a.grid, NZ), dim3(NWV * 64), LDS, st, a);
    RV_LAUNCH_CHECK();
    return 0;
}

// the A/B knob of this process, read once
static const C24Knobs& c24_knobs() {
    static const C24Knobs knobs = c24_knobs_from_env();
    return knobs;
}

// what a plan outside RV_C24_VARIANTS is reported with
static const char* c24_no_kernel(const C24Plan& p) { return p.no_twin ? p.no_twin : "conv24: no kernel for this plan"; }

// the launch of a plan with its filled arguments
static int c24_dispatch(C24Args& a, const C24Plan& p, void* stream) {
    switch (p.key()) {                                             // key and launcher of a case: the same entry of RV_C24_VARIANTS (fixed_plan.h)
#define RV_C24_CASE(...) case c24_variant_key(__VA_ARGS__): return launch_c24<__VA_ARGS__>(a, p, (hipStream_t)stream);
        RV_C24_VARIANTS(RV_C24_CASE)
#undef RV_C24_CASE
    }
    RV_CHECK(false, "%s", c24_no_kernel(p));
    return 1;
}

// Test query (refvsr_hip.h): the plan an entry point would launch, by c24_plan under c24_knobs() -- the function and the knob object
// of the entry points above.  Host only: no launch, no refvsr_init, no HIP call
extern "C" int refvsr_conv24_variant(int op, int x0, int x1, int mm, int wf, int batch, int h, int w, long long* key, int* n_tiles, int* lds) {
    RV_CHECK(key != nullptr, "conv24_variant: null key");
    RV_CHECK(op >= C24_CONV24 && op <= C24_CONV_LAST && (mm == 0 || mm == 1) && (wf == 0 || wf == 1) && h > 0 && w > 0, "conv24_variant: bad args");
    C24Plan p;
    if (int rc = c24_plan((C24Op)op, x0, x1, mm, wf, mm ? batch : 1, h, w, c24_knobs(), &p)) return rc;
    bool listed = false;
    switch (p.key()) {
#define RV_C24_CASE(...) case c24_variant_key(__VA_ARGS__):
        RV_C24_VARIANTS(RV_C24_CASE) listed = !p.no_twin;
#undef RV_C24_CASE
    }
    RV_CHECK(listed, "%s", c24_no_kernel(p));
    *key = p.key();
    if (n_tiles) *n_tiles = p.n_tiles;
    if (lds) *lds = p.lds;
    return 0;
}

extern "C" int refvsr_conv24_supported(int c0, int c1) { return c24_supported(C24_CONV24, c0, c1); }
extern "C" int refvsr_conv48_supported(int c0, int c1) { return c24_supported(C24_CONV48, c0, c1); }
extern "C" int refvsr_conv32_supported(int c0, int c1) { return c24_supported(C24_CONV32, c0, c1); }
extern "C" int refvsr_conv_shuffle2_supported(int c) { return c24_supported(C24_SHUFFLE2, c, 0); }

// Blob sizes (fixed_plan.h:c24_blob_bytes).  48 + 48: two channel-half blobs of the 24-output layout, back to back; pixel shuffle: one
// 48-row blob per row group.  The fp16 weight format (ABI 15, refvsr_*_f16w; packing.py:pack_conv24 / pack_conv_shuffle2 with
// wfmt='fp16') has c24_nf(cout, 1) fragments per K-step and the same bias tail; the twins exist for the shapes the mid_channels = 24
// family launches.
extern "C" int refvsr_conv24_blob_bytes(int c0, int c1) { return refvsr_conv24_supported(c0, c1) ? c24_blob_bytes(24, (c0 + c1) / 8, 0) : -1; }
extern "C" int refvsr_conv32_blob_bytes(int c0, int c1) { return refvsr_conv32_supported(c0, c1) ? c24_blob_bytes(32, (c0 + c1) / 8, 0) : -1; }
extern "C" int refvsr_conv48_blob_bytes(int c0, int c1) {
    if (!refvsr_conv48_supported(c0, c1)) return -1;
    return c0 == 48 && c1 == 48 ? c24_nz(0, 1) * c24_blob_bytes(24, 12, 0) : c24_blob_bytes(48, (c0 + c1) / 8, 0);
}
extern "C" int refvsr_conv_shuffle2_blob_bytes(int c) { return refvsr_conv_shuffle2_supported(c) ? c24_nz(c, 0) * c24_blob_bytes(48, c / 8, 0) : -1; }
extern "C" int refvsr_conv24_f16w_blob_bytes(int c0, int c1) { return refvsr_conv24_supported(c0, c1) ? c24_blob_bytes(24, (c0 + c1) / 8, 1) : -1; }
extern "C" int refvsr_conv32_f16w_blob_bytes(int c0, int c1) { return refvsr_conv32_supported(c0, c1) ? c24_blob_bytes(32, (c0 + c1) / 8, 1) : -1; }
extern "C" int refvsr_conv_shuffle2_f16w_blob_bytes(int c) { return c == 24 ? c24_nz(c, 0) * c24_blob_bytes(48, c / 8, 1) : -1; }

extern "C" int refvsr_conv24_kblock(int ncg, int s, int q) {
    if (c24_steps(ncg) == 0 || s < 0 || s >= c24_steps(ncg) || q < 0 || q > 3) return -2;
    return c24_kblock(ncg, s, q);
}

static int c24_fill(C24Args& a, const char* who, int cout, const void* src0, const void* src1, int c1, int h, int w, const void* blob,
                    float act_slope, const void* mul, const void* res, float post_slope, void* out) {
    RV_CHECK(src0 && out && blob && h > 0 && w > 0, "%s: bad args", who);
    RV_CHECK((c1 == 0) == (src1 == nullptr), "%s: src1 / c1 mismatch", who);
    RV_CHECK(((uintptr_t)blob & 15) == 0, "%s: blob must be 16-byte aligned", who);
    RV_CHECK(act_slope >= 0.f && act_slope <= 1.f && post_slope >= 0.f && post_slope <= 1.f, "%s: activation slopes must lie in [0, 1]", who);
    RV_CHECK(src0 != out && src1 != out, "%s: in-place operation is not supported", who);
    RV_CHECK((long long)h * w * cout * 2 < (1ll << 31), "%s: map too large for 32-bit offsets", who);
    RV_CHECK(refvsr_init() == 0, "init failed");
    memset(&a, 0, sizeof(a));
    a.src0 = (const unsigned char*)src0; a.src1 = (const unsigned char*)src1; a.out = (unsigned char*)out;
    a.blob = (const unsigned char*)blob; a.mul = (const unsigned char*)mul; a.res = (const unsigned char*)res;
    a.h = h; a.w = w; a.act_slope = act_slope; a.post_slope = post_slope;
    return 0;
}

// Per-map operands of an entry point (ABI 11): `batch` device pointers per operand in host arrays; a single-map entry passes the
// addresses of its own arguments and batch = 1.  The checks of c24_fill on map 0, then every map's null / alias checks and the
// per-map tables the MM = 1 kernels read.
static int c24_fill_maps(C24Args& a, const char* who, int cout, const void* const* src0, const void* const* src1, int c1, int batch,
                         int h, int w, const void* blob, float act_slope, const void* const* mul, const void* const* res,
                         float post_slope, void* const* out) {
    if (c24_fill(a, who, cout, src0[0], src1 ? src1[0] : nullptr, c1, h, w, blob, act_slope, mul ? mul[0] : nullptr,
                 res ? res[0] : nullptr, post_slope, out[0])) return 1;
    a.batch = batch;
    for (int b = 0; b < batch; ++b) {
        RV_CHECK(src0[b] && out[b] && (!src1 || src1[b]) && (!mul || mul[b]) && (!res || res[b]), "%s: null map pointer (map %d)", who, b);
        for (int c = 0; c < batch; ++c)
            RV_CHECK(src0[c] != out[b] && (!src1 || src1[c] != out[b]) && (c == b || out[c] != out[b]), "%s: in-place operation is not supported", who);
        a.bsrc0[b] = (const unsigned char*)src0[b]; a.bsrc1[b] = src1 ? (const unsigned char*)src1[b] : nullptr;
        a.bout[b] = (unsigned char*)out[b];
        a.bmul[b] = mul ? (const unsigned char*)mul[b] : nullptr; a.bres[b] = res ? (const unsigned char*)res[b] : nullptr;
    }
    return 0;
}
// a single-map entry's optional operand as a one-entry table
#define C24_OPT(p) ((p) ? &(p) : nullptr)

// Each op below: ONE implementation (wf, mm) over per-map tables -- plan (fixed_plan.h:c24_plan: shape support, kernel variant, tile
// counts), argument checks and fill, c24_dispatch.  mm = 0: the single-map entry (its own arguments, batch = 1); mm = 1: the `_batch`
// entry (ABI 11), `batch` maps of one geometry in ONE launch of the multi-map kernel.  wf = 1: the `_f16w` twin.
static int c24_conv24(int wf, int mm, const void* const* src0, int c0, const void* const* src1, int c1, int batch, int h, int w, const void* blob,
                      float act_slope, const void* const* mul, const void* const* res, float post_slope, void* const* out, void* stream) {
    const char* who = mm ? "conv24_batch" : "conv24";
    C24Plan p;
    C24Args a;
    if (c24_plan(C24_CONV24, c0, c1, mm, wf, batch, h, w, c24_knobs(), &p)) return 1;
    RV_CHECK(src0 && out, "%s: 1..%d maps per launch", who, REFVSR_MAX_MAPS);
    RV_CHECK(!mm || (c1 == 0) == (src1 == nullptr), "%s: src1 / c1 mismatch", who);
    if (c24_fill_maps(a, who, 24, src0, src1, c1, batch, h, w, blob, act_slope, mul, res, post_slope, out)) return 1;
    return c24_dispatch(a, p, stream);
}
#define C24_CONV_ARGS const void* src0, int c0, const void* src1, int c1, int h, int w, const void* blob, float act_slope, \
                      const void* mul, const void* res, float post_slope, void* out, void* stream
#define C24_CONV_BATCH_ARGS const void* const* src0, int c0, const void* const* src1, int c1, int batch, int h, int w, const void* blob, \
                            float act_slope, const void* const* mul, const void* const* res, float post_slope, void* const* out, void* stream
#define C24_CONV_PASS(WF) c24_conv24(WF, 0, &src0, c0, C24_OPT(src1), c1, 1, h, w, blob, act_slope, C24_OPT(mul), C24_OPT(res), post_slope, &out, stream)
#define C24_CONV_BATCH_PASS(WF) c24_conv24(WF, 1, src0, c0, src1, c1, batch, h, w, blob, act_slope, mul, res, post_slope, out, stream)
extern "C" int refvsr_conv24(C24_CONV_ARGS) { return C24_CONV_PASS(0); }
extern "C" int refvsr_conv24_f16w(C24_CONV_ARGS) { return C24_CONV_PASS(1); }
extern "C" int refvsr_conv24_batch(C24_CONV_BATCH_ARGS) { return C24_CONV_BATCH_PASS(0); }
extern "C" int refvsr_conv24_batch_f16w(C24_CONV_BATCH_ARGS) { return C24_CONV_BATCH_PASS(1); }

// 32 output channels (AlignedConv2d, RefVSR_/alignment.py:18-24,53-100: the 3 -> 32 stem and the 32 -> 32 convs of its ResBlocks) and 48
// (the mid_channels = 48 family; hi + lo weights only)
static int c24_conv_single(C24Op op, const char* who, int cout, int wf, C24_CONV_ARGS) {
    C24Plan p;
    C24Args a;
    if (c24_plan(op, c0, c1, 0, wf, 1, h, w, c24_knobs(), &p)) return 1;
    if (c24_fill(a, who, cout, src0, src1, c1, h, w, blob, act_slope, mul, res, post_slope, out)) return 1;
    return c24_dispatch(a, p, stream);
}
#define C24_CONV_SINGLE(OP, WHO, COUT, WF) c24_conv_single(OP, WHO, COUT, WF, src0, c0, src1, c1, h, w, blob, act_slope, mul, res, post_slope, out, stream)
extern "C" int refvsr_conv32(C24_CONV_ARGS) { return C24_CONV_SINGLE(C24_CONV32, "conv32", 32, 0); }
extern "C" int refvsr_conv32_f16w(C24_CONV_ARGS) { return C24_CONV_SINGLE(C24_CONV32, "conv32", 32, 1); }
extern "C" int refvsr_conv48(C24_CONV_ARGS) { return C24_CONV_SINGLE(C24_CONV48, "conv48", 48, 0); }

// act(C -> 4 C 3x3 conv + bias) through F.pixel_shuffle(2) on fp16 HWC maps: src [h][w][C] -> out [2h][2w][C].  blobs: the 2 (C = 24) or
// 4 (C = 48) row-group blobs of refvsr_amd/packing.py:pack_conv_shuffle2, back to back.  The `_batch` entries (PixelShufflePack over
// `batch` maps: upsample1 of the RAP steps, RefVSR.py:138) and the `_f16w` twins take C = 24 only.
static int c24_conv_shuffle2(int wf, int mm, const void* const* src, int batch, int c, int h, int w, const void* blobs, float act_slope,
                             void* const* out, void* stream) {
    const char* who = mm ? "conv_shuffle2_batch" : "conv_shuffle2";
    C24Plan p;
    C24Args a;
    if (c24_plan(C24_SHUFFLE2, c, 0, mm, wf, batch, h, w, c24_knobs(), &p)) return 1;
    RV_CHECK(src && out, "%s: 1..%d maps per launch", who, REFVSR_MAX_MAPS);
    if (c24_fill_maps(a, who, 4 * c, src, nullptr, 0, batch, h, w, blobs, act_slope, nullptr, nullptr, 1.0f, out)) return 1;   // (4 c: the 2h x 2w x c output map)
    return c24_dispatch(a, p, stream);
}
#define C24_SHUF_ARGS const void* src, int c, int h, int w, const void* blobs, float act_slope, void* out, void* stream
#define C24_SHUF_BATCH_ARGS const void* const* src, int batch, int c, int h, int w, const void* blobs, float act_slope, void* const* out, void* stream
extern "C" int refvsr_conv_shuffle2(C24_SHUF_ARGS) { return c24_conv_shuffle2(0, 0, &src, 1, c, h, w, blobs, act_slope, &out, stream); }
extern "C" int refvsr_conv_shuffle2_f16w(C24_SHUF_ARGS) { return c24_conv_shuffle2(1, 0, &src, 1, c, h, w, blobs, act_slope, &out, stream); }
extern "C" int refvsr_conv_shuffle2_batch(C24_SHUF_BATCH_ARGS) { return c24_conv_shuffle2(0, 1, src, batch, c, h, w, blobs, act_slope, out, stream); }
extern "C" int refvsr_conv_shuffle2_batch_f16w(C24_SHUF_BATCH_ARGS) { return c24_conv_shuffle2(1, 1, src, batch, c, h, w, blobs, act_slope, out, stream); }

// The confidence fusions of AA_AF_conf_prop / compute_up in ONE launch (RefVSR.py:47-52 conf_fusion / conf_fusion2 /
// conf_fusion_BWFW, called at :130, :141-142, :107-109):
//   alpha = lrelu_{slope1}( conv3x3_{16 -> cout}( lrelu_{slope0}( conv3x3_{2 -> 16}( P ) ) ) ),
//   P = cat[conf_a, conf_b]  (up = 1)   |   clamp01( F.interpolate(cat[conf_a, conf_b], x2, bicubic) )  (up = 2),
// both convs zero padded.  conf_a / conf_b: planar fp32 [h][w]; w0 / b0: fp32 [16][2][3][3] / [16] (device); blob: the 16 -> cout
// blob of refvsr_conv24 / refvsr_conv48 (cout = 24 | 48); alpha: fp16 HWC [up h][up w][cout]; conf_max (optional, up = 1):
// max(conf_a, conf_b) [h][w] (RefVSR.py:147).  Bit-identical to torch.cat + [refvsr_resize +] refvsr_conv_direct_f32 +
// refvsr_conv24 / 48 [+ refvsr_max2].  The `_batch` entries (`batch` pairs of maps) and the `_f16w` twins take cout = 24 only.
static int c24_conf_alpha(int wf, int mm, const float* const* conf_a, const float* const* conf_b, int batch, int h, int w, int up, const float* w0,
                          const float* b0, float slope0, const void* blob, int cout, float slope1, void* const* alpha,
                          float* const* conf_max, void* stream) {
    const char* who = mm ? "conf_alpha_batch" : "conf_alpha";
    if (mm) RV_CHECK(conf_a && conf_b && w0 && b0 && alpha, "conf_alpha_batch: bad args (1..%d maps)", REFVSR_MAX_MAPS);
    else RV_CHECK(conf_a[0] && conf_b[0] && w0 && b0 && alpha[0], "conf_alpha: null argument");
    C24Plan p;
    C24Args a;
    if (c24_plan(C24_CONF_ALPHA, cout, up, mm, wf, batch, h, w, c24_knobs(), &p)) return 1;
    RV_CHECK(conf_max == nullptr || up == 1, "%s: the max by-product exists at up = 1 only", who);
    RV_CHECK(slope0 >= 0.f && slope0 <= 1.f, "%s: activation slopes must lie in [0, 1]", who);
    if (c24_fill(a, who, cout, conf_a[0], nullptr, 0, up * h, up * w, blob, slope1, nullptr, nullptr, 1.0f, alpha[0])) return 1;
    a.src0 = nullptr;
    a.conf_a = conf_a[0]; a.conf_b = conf_b[0]; a.cw0 = w0; a.cb0 = b0; a.conf_max = conf_max ? conf_max[0] : nullptr; a.ch = h; a.cw = w; a.slope0 = slope0;
    a.batch = batch;
    for (int b = 0; b < batch; ++b) {
        RV_CHECK(conf_a[b] && conf_b[b] && alpha[b] && (!conf_max || conf_max[b]), "%s: null map pointer (map %d)", who, b);
        a.bconf_a[b] = conf_a[b]; a.bconf_b[b] = conf_b[b]; a.bconf_max[b] = conf_max ? conf_max[b] : nullptr;
        a.bout[b] = (unsigned char*)alpha[b];
    }
    return c24_dispatch(a, p, stream);
}
#define C24_CONF_ARGS const float* conf_a, const float* conf_b, int h, int w, int up, const float* w0, const float* b0, float slope0, \
                      const void* blob, int cout, float slope1, void* alpha, float* conf_max, void* stream
#define C24_CONF_BATCH_ARGS const float* const* conf_a, const float* const* conf_b, int batch, int h, int w, int up, const float* w0, const float* b0, \
                            float slope0, const void* blob, int cout, float slope1, void* const* alpha, float* const* conf_max, void* stream
#define C24_CONF_PASS(WF) c24_conf_alpha(WF, 0, &conf_a, &conf_b, 1, h, w, up, w0, b0, slope0, blob, cout, slope1, &alpha, C24_OPT(conf_max), stream)
#define C24_CONF_BATCH_PASS(WF) c24_conf_alpha(WF, 1, conf_a, conf_b, batch, h, w, up, w0, b0, slope0, blob, cout, slope1, alpha, conf_max, stream)
extern "C" int refvsr_conf_alpha(C24_CONF_ARGS) { return C24_CONF_PASS(0); }
extern "C" int refvsr_conf_alpha_f16w(C24_CONF_ARGS) { return C24_CONF_PASS(1); }
extern "C" int refvsr_conf_alpha_batch(C24_CONF_BATCH_ARGS) { return C24_CONF_BATCH_PASS(0); }
extern "C" int refvsr_conf_alpha_batch_f16w(C24_CONF_BATCH_ARGS) { return C24_CONF_BATCH_PASS(1); }

// The output head in ONE launch (RefVSR.py:92,118,288,297: conv_last 3x3 C -> 3, + F.interpolate(lr_centre, scale, bicubic).clamp(0, 1),
// final clamp): out planar fp32 [3][h][w] = clamp( conv(src) + bias + clamp01(bicubic(base_lr)), 0, 1 ).  src: fp16 HWC [h][w][c],
// c = 24 | 48; base_lr: planar fp32 [3][bh][bw] with h / bh == w / bw the SR factor of this stage; blob: refvsr_conv_last_blob_bytes(c)
// bytes = [S K-steps x ONE fragment x 64 lanes x 8 halfs][32 bias floats]: fragment rows 0-2 = hi(W[r]), rows 8-10 = lo(W[r - 8]),
// K-blocks by refvsr_conv24_kblock(c / 8, s, q) (refvsr_amd/packing.py:pack_conv_last).  Replaces refvsr_resize (the x4 base map)
// + refvsr_conv_mfma's planar mode: the 3-channel base never exists in HBM, one MFMA per K-step instead of two 16-row tiles.
extern "C" int refvsr_conv_last_supported(int c) { return c24_supported(C24_CONV_LAST, c, 0); }
extern "C" int refvsr_conv_last_blob_bytes(int c) { return refvsr_conv_last_supported(c) ? c24_blob_bytes(3, c / 8, 0) : -1; }
extern "C" int refvsr_conv_last_fmt(const void* src, int c, int h, int w, const void* blob, const float* base_lr, int bh, int bw,
                                    void* out, int out_fmt, void* stream);
extern "C" int refvsr_conv_last(const void* src, int c, int h, int w, const void* blob, const float* base_lr, int bh, int bw,
                                float* out, void* stream) {
    return refvsr_conv_last_fmt(src, c, h, w, blob, base_lr, bh, bw, out, REFVSR_RESULT_F32, stream);
}
extern "C" int refvsr_conv_last_fmt(const void* src, int c, int h, int w, const void* blob, const float* base_lr, int bh, int bw,
                                    void* out, int out_fmt, void* stream) {
    RV_CHECK(rv_result_fmt_ok(out_fmt), "conv_last: unknown result format %d", out_fmt);
    C24Plan p;
    C24Args a;
    if (c24_plan(C24_CONV_LAST, c, 0, 0, 0, 1, h, w, c24_knobs(), &p)) return 1;
    RV_CHECK(base_lr && bh > 0 && bw > 0 && h % bh == 0 && w % bw == 0 && h / bh == w / bw, "conv_last: base frame %dx%d does not divide the output %dx%d", bh, bw, h, w);
    if (c24_fill(a, "conv_last", c, src, nullptr, 0, h, w, blob, 1.0f, nullptr, nullptr, 1.0f, out)) return 1;
    a.base_lr = base_lr; a.bh = bh; a.bw = bw; a.base_step = (float)bh / (float)h; a.out_fmt = out_fmt;
    return c24_dispatch(a, p, stream);
}
