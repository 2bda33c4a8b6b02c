// Launch plan of the generic MFMA convolution (conv_mfma.hip): every check of a RefvsrConv descriptor and the choice of the
// conv_mfma_kernel<MT, TILES, F32, GATHER, RESIDENT, EPI, NW, HI1> instantiation with its LDS carve, as a pure function of the
// descriptor and the A/B knobs.  No HIP call, no device query: it also compiles with a plain host compiler, which is how
// tests/test_conv_plan.py pins it (tools/conv_plan_dump.cpp).  What depends on the device -- the grid cap of the persistent
// kernels -- stays with the launcher.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include "../../include/refvsr_hip.h"
#include "plan_common.h"

#define CONV_CH 8          // K-steps of weights per streamed LDS chunk (chunked convs)
#define CONV_RES_MAX 16    // K-steps a resident weight set may have (persistent convs)
#define CONV_XPF 8         // uint4 prefetch registers per thread for the next input tile (persistent convs)
#define CONV_TW 32         // output tile width in pixels

// Every instantiation of conv_mfma_kernel, X(MT, TILES, F32, GATHER, RESIDENT, EPI, NW, HI1): the ONLY place where they are written
// down.  conv_mfma.hip expands the list into its dispatch (a switch on the key: a list entry twice is a compile error), host-only
// code into the list of keys.
#define RV_CONV_VARIANTS(X)                                                                                          \
    /* gather mode (fp16 strided predictors) */                                                                      \
    X(1, 4, false, true, false, 0, 4, false) X(2, 4, false, true, false, 0, 4, false) X(3, 4, false, true, false, 0, 4, false) \
    /* single-fp16 weights, streamed: 8 waves | 8 x 32 | 4 x 32 */                                                   \
    X(1, 2, false, false, false, 0, 8, true) X(2, 2, false, false, false, 0, 8, true)                                \
    X(1, 4, false, false, false, 0, 4, true) X(2, 4, false, false, false, 0, 4, true)                                \
    X(1, 2, false, false, false, 0, 4, true) X(2, 2, false, false, false, 0, 4, true)                                \
    /* 16 x 32 tile, 16 waves, resident */                                                                           \
    X(3, 2, false, false, true, 1, 16, false) X(3, 2, false, false, true, 0, 16, false)                              \
    X(2, 2, false, false, true, 1, 16, false) X(2, 2, false, false, true, 0, 16, false)                              \
    /* 8 x 32 tile, 8 waves: lean | resident | streamed */                                                           \
    X(1, 2, false, false, true, 1, 8, false) X(1, 2, false, false, true, 0, 8, false) X(1, 2, false, false, false, 0, 8, false) \
    X(2, 2, false, false, true, 1, 8, false) X(2, 2, false, false, true, 0, 8, false) X(2, 2, false, false, false, 0, 8, false) \
    X(3, 2, false, false, true, 1, 8, false) X(3, 2, false, false, true, 0, 8, false) X(3, 2, false, false, false, 0, 8, false) \
    /* fp32, 4 x 32 tile, 8 waves */                                                                                 \
    X(1, 1, true, false, true, 0, 8, false) X(1, 1, true, false, false, 0, 8, false)                                 \
    X(2, 1, true, false, true, 0, 8, false) X(2, 1, true, false, false, 0, 8, false)                                 \
    /* 4 waves, (MT, TILES) = (1..3, 2 | 4): fp32 resident | fp32 streamed | lean | resident | streamed */           \
    RV_CONV_VARIANTS4(X, 1, 2) RV_CONV_VARIANTS4(X, 1, 4) RV_CONV_VARIANTS4(X, 2, 2) RV_CONV_VARIANTS4(X, 2, 4)     \
    RV_CONV_VARIANTS4(X, 3, 2) RV_CONV_VARIANTS4(X, 3, 4)
#define RV_CONV_VARIANTS4(X, M, T)                                                                                   \
    X(M, T, true, false, true, 0, 4, false) X(M, T, true, false, false, 0, 4, false)                                 \
    X(M, T, false, false, true, 1, 4, false) X(M, T, false, false, true, 0, 4, false) X(M, T, false, false, false, 0, 4, false)

// the template arguments packed into one integer: what a plan is looked up by
constexpr int conv_variant_key(int MT, int TILES, bool F32, bool GATHER, bool RESIDENT, int EPI, int NW, bool HI1) {
    return MT | TILES << 2 | NW << 6 | EPI << 11 | (int)F32 << 12 | (int)GATHER << 13 | (int)RESIDENT << 14 | (int)HI1 << 15;
}

// A/B knobs of the generic conv (README: the REFVSR_CONV_* table); the defaults are the shipped behaviour
struct ConvKnobs {
    bool no_persist = false;         // REFVSR_CONV_NO_PERSIST: no resident (persistent) kernels
    int res_max = CONV_RES_MAX;      // REFVSR_CONV_RES_MAX: K-steps a resident weight set may have (at most CONV_RES_MAX)
    int tiles = 0;                   // REFVSR_CONV_TILES: 2 | 4 forces the resident tile height (0: chosen)
    bool no_w16 = false;             // REFVSR_CONV_NO_W16: no 16 x 32 tiles on 16 waves
    int ring = 0;                    // REFVSR_CONV_RING: 2 | 3 | 4 caps the LDS ring of the streamed kernels (0: what fits)
    bool no_nw8 = false;             // REFVSR_CONV_NO_NW8: no 8-wave workgroups
    bool no_prefetch = false;        // REFVSR_CONV_NO_PREFETCH: resident kernels do not prefetch the next tile
    bool no_lean_epi = false;        // REFVSR_CONV_NO_LEAN_EPI: general epilogue everywhere
};
static inline ConvKnobs conv_knobs_from_env() {
    ConvKnobs k;
    auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    k.no_persist = getenv("REFVSR_CONV_NO_PERSIST") != nullptr;
    k.res_max = num("REFVSR_CONV_RES_MAX", CONV_RES_MAX);
    k.tiles = num("REFVSR_CONV_TILES", 0);
    k.no_w16 = getenv("REFVSR_CONV_NO_W16") != nullptr;
    k.ring = num("REFVSR_CONV_RING", 0);
    k.no_nw8 = getenv("REFVSR_CONV_NO_NW8") != nullptr;
    k.no_prefetch = getenv("REFVSR_CONV_NO_PREFETCH") != nullptr;
    k.no_lean_epi = getenv("REFVSR_CONV_NO_LEAN_EPI") != nullptr;
    return k;
}

struct ConvPlan {
    int MT, TILES; bool F32, GATHER, RESIDENT; int EPI, NW; bool HI1;   // the instantiation
    int nz;                          // gridDim.z: groups of MT sixteen-row tiles
    size_t lds;                      // dynamic LDS: [table][weights: resident set | ring][input tile]
    int tab_bytes, wl_bytes;         // LDS carve sizes
    int ring;                        // streamed kernels: LDS ring slots of CONV_CH K-steps each (2..4; gather mode: 1)
    int LH, LW;                      // LDS input tile extent in pixels (gather mode: 0)
    int ps;                          // LDS pixel stride in 16-byte slots (odd)
    int G, S;                        // valid K-blocks, K-steps
    int tiles_x, n_xy;               // pixel tiles per row / per frame
    int gather;                      // 1: no LDS input tile, B fragments gathered from global memory
    int prefetch;                    // resident kernels: 1 = next tile prefetched into registers during the K loop
    int key() const { return conv_variant_key(MT, TILES, F32, GATHER, RESIDENT, EPI, NW, HI1); }
};

// 0 and *p filled, or 1 and the message set (refvsr_set_error)
static int conv_plan(const RefvsrConv* d, const ConvKnobs& knobs, ConvPlan* p) {
    RV_CHECK(d != nullptr, "conv: null descriptor");
    *p = ConvPlan();
    const bool f32 = d->f32 == 1;
    const bool hi1 = d->f32 == 2;                      // fp16 weights without the lo term (streamed kernels only)
    RV_CHECK(d->f32 >= 0 && d->f32 <= 2, "conv: weight mode (f32) must be 0, 1 or 2");
    const int cgrp = f32 ? 4 : 8;                      // channels per 16-byte group
    RV_CHECK(d->src0 && d->c0 > 0 && d->c0 % cgrp == 0, "conv: src0/c0 invalid (c0=%d)", d->c0);
    RV_CHECK((d->src1 == nullptr) == (d->c1 == 0) && d->c1 % cgrp == 0, "conv: src1/c1 invalid (c1=%d)", d->c1);
    RV_CHECK(d->ksize >= 1 && d->ksize <= 7 && d->stride >= 1 && d->pad >= 0, "conv: bad geometry");
    RV_CHECK(d->h_in > 0 && d->w_in > 0 && d->h_out > 0 && d->w_out > 0, "conv: bad sizes");
    RV_CHECK(d->wpack && d->bias && d->out, "conv: null weights/bias/out");
    RV_CHECK(d->mt_per_block >= 1 && d->mt_per_block <= 3, "conv: mt_per_block must be 1..3");
    RV_CHECK(d->cout >= 1, "conv: cout");
    if (d->out_mode != REFVSR_OUT_PLANAR32) {
        RV_CHECK(d->cout % 4 == 0 && d->out_c % 4 == 0, "conv: nhwc16 output needs cout %% 4 == 0");
        RV_CHECK(d->res_planar == nullptr, "conv: res_planar only with planar output");
    }
    if (d->out_mode == REFVSR_OUT_NHWC16_SHUFFLE2)
        RV_CHECK(d->cout % 16 == 0 && !d->mul && !d->res && !f32 && d->out_c >= d->cout / 4 && d->out_c - d->cout / 4 <= 4,
                 "conv: pixel-shuffle output constraints");
    const int ncg = (d->c0 + d->c1) / cgrp, ks = d->ksize, stride = d->stride;
    p->ps = ncg | 1;
    p->G = ks * ks * ncg;
    p->S = rv_ksteps(ks, ncg);
    RV_CHECK(p->S == d->ksteps, "conv: ksteps mismatch (descriptor %d, geometry %d)", d->ksteps, p->S);
    RV_CHECK(d->batch >= 0 && d->batch <= 65535, "conv: batch out of range (%d)", d->batch);
    if (d->batch > 1) {
        RV_CHECK(!d->mul && !d->res, "conv: batch > 1 takes no mul / res operands");
        RV_CHECK(d->bs_src0 % 16 == 0 && d->bs_src1 % 16 == 0 && d->bs_out % 8 == 0 && d->bs_res_planar % 4 == 0, "conv: batch strides must keep the maps aligned");
        RV_CHECK(d->bs_src0 > 0 && d->bs_out > 0 && (!d->src1 || d->bs_src1 > 0) && (!d->res_planar || d->bs_res_planar > 0), "conv: batch strides missing");
    }

    const int MT = d->mt_per_block, S = p->S;
    p->nz = rv_cdiv(rv_cdiv(d->cout, 16), MT);
    p->tab_bytes = ((S * 4 * 4 + 15) / 16) * 16;
    const int wfr_kb = MT * ((f32 || hi1) ? 1 : 2) * 1024;   // bytes of weight fragments per K-step
    const size_t LDS_MAX = 160 * 1024;

    int tiles = 4;                                     // the tile is 2 * tiles rows x 32 pixels
    size_t lds = 0;
    auto tile_bytes = [&](int tl) {
        p->LH = (tl * 2 - 1) * stride + ks;
        p->LW = (CONV_TW - 1) * stride + ks;
        return (size_t)p->LH * p->LW * p->ps * 16;
    };
    // RESIDENT: whole weight set in LDS, persistent workgroups with a register-prefetched input tile.  Needs few enough
    // K-steps, a tile that fits the prefetch registers, and LDS for >= 2 workgroups per CU (8 x 32 pixels preferred,
    // 4 x 32 when that buys a second / third workgroup).
    bool resident = false, one_wg = false;             // one_wg: LDS admits a single workgroup per CU
    bool w16 = false;                                  // 16 x 32 tile, 16 waves
    if (!knobs.no_persist && !hi1 && S <= knobs.res_max && S <= CONV_RES_MAX) {
        int best_wg = 0;
        for (int tl = 4; tl >= 2; tl -= 2) {
            if (knobs.tiles && tl != knobs.tiles) continue;
            const size_t tb = tile_bytes(tl);
            const size_t need = (size_t)p->tab_bytes + (size_t)S * wfr_kb + tb;
            const int chunks = p->LH * p->LW * ncg;
            const int wg = need <= LDS_MAX ? (int)(LDS_MAX / need) : 0;
            if (chunks > CONV_XPF * 256 || wg == 0) continue;
            if (p->LH > 31 || p->LW > 127 || ncg > 127) continue;   // packed chunk descriptor of the tile staging (r:5, c:7, cg:7 + 7 bits)
            if (best_wg == 0 || (best_wg < 2 && wg > best_wg)) { best_wg = wg; tiles = tl; lds = need; resident = true; }
        }
        if (resident) { p->wl_bytes = S * wfr_kb; tile_bytes(tiles); one_wg = best_wg == 1; }
        // One workgroup per CU (the C = 48 weight sets): a 16 x 32 tile walked by SIXTEEN waves (two pixel groups each) keeps
        // four waves per SIMD next to the 84 KB weight set and halves the halo; 8 waves on 8 x 32 where that does not fit.
        // (same box, frames/s: RefVSR_MFID 60.6 [4 waves] / 68.9 [8 x 2] / 70.1 [8 x 4] / 72.2 [16 x 2]; MFID_8K 1080p 5.04 / 5.80 / 6.24 / 6.25)
        if (resident && one_wg && tiles == 4 && !f32 && !knobs.no_w16 && (MT == 2 || MT == 3)) {
            const size_t tb = tile_bytes(8);
            const size_t need = (size_t)p->tab_bytes + (size_t)S * wfr_kb + tb;
            const int chunks = p->LH * p->LW * ncg;
            if (need <= LDS_MAX && chunks <= 4096 && p->LH <= 31 && p->LW <= 127) { tiles = 8; lds = need; w16 = true; }
            else tile_bytes(tiles);
        }
    }
    if (!resident) {
        // streamed weights: a ring of 2..4 LDS slots of CONV_CH K-steps each next to the staged input tile.  Large maps prefer a
        // footprint that admits two workgroups per CU; 8 x 32 pixels if the staged input fits, else 4 x 32, else gather mode
        // (one slot, register-prefetched, B fragments from global memory)
        const size_t slot = (size_t)CONV_CH * wfr_kb;
        const int n_chunks = (S + CONV_CH - 1) / CONV_CH;
        auto ring_for = [&](int tl, size_t budget) {
            const size_t fixed = (size_t)p->tab_bytes + tile_bytes(tl);
            if (fixed + 2 * slot > budget) return 0;
            int ns = (int)((budget - fixed) / slot);
            if (ns > 4) ns = 4;
            if (ns > n_chunks + 1) ns = n_chunks + 1 > 2 ? n_chunks + 1 : 2;
            return ns;
        };
        const bool big = (long long)d->h_out * d->w_out > 64 * 1024;
        int ns = 0;
        tiles = 4;
        if (big) ns = ring_for(4, LDS_MAX / 2);
        if (!ns && big) { tiles = 2; ns = ring_for(2, LDS_MAX / 2); }
        if (!ns) { tiles = 4; ns = ring_for(4, LDS_MAX); }
        if (!ns) { tiles = 2; ns = ring_for(2, LDS_MAX); }
        if (ns) {
            if (knobs.ring >= 2 && knobs.ring < ns) ns = knobs.ring;
            p->ring = ns;
            p->wl_bytes = (int)(ns * slot);
            lds = (size_t)p->tab_bytes + (size_t)p->wl_bytes + tile_bytes(tiles);
        } else {                                       // strided predictor convs: gather B fragments from global memory
            p->gather = 1;
            p->ring = 1;
            tiles = 4;
            p->LH = p->LW = 0;
            p->wl_bytes = (int)slot;
            lds = (size_t)p->tab_bytes + (size_t)p->wl_bytes;
            RV_CHECK(d->h_in < 60000 && d->w_in < 60000, "conv: frame too large for gather-mode coordinates");
        }
        one_wg = !p->gather && lds > LDS_MAX / 2;
    }
    p->lds = lds;
    p->prefetch = knobs.no_prefetch ? 0 : 1;
    p->tiles_x = rv_cdiv(d->w_out, CONV_TW);
    p->n_xy = p->tiles_x * rv_cdiv(d->h_out, tiles * 2);

    // ---- the instantiation: 4 waves with `tiles` pixel groups each unless one of the rules below says otherwise
    p->MT = MT; p->TILES = tiles; p->F32 = f32; p->GATHER = p->gather != 0; p->RESIDENT = resident; p->EPI = 0; p->NW = 4; p->HI1 = hi1;
    // nw8 -- one workgroup per CU: eight waves on the same 8 x 32 tile (two pixel groups per wave) keep two waves per SIMD;
    // and eight waves (two pixel groups each) on the other 8 x 32 fp16 tiles as well, unless the map is large: 2 workgroups x
    // 8 waves = 4 waves per SIMD instead of 3 x 4 = 3 hides more latency (24->24 at 270p 9.7 -> 9.2 us, at 540p 24.3 -> 23.0 us,
    // same box 156.7 -> 159.3 frames/s on RefVSR_small); at 1080p (4080 tiles, 8 per workgroup) the better weight-fragment
    // reuse of four pixel groups per wave wins (75.5 vs 78.5 us).  (Forcing <= 80 VGPRs for 6 waves per SIMD spills.)
    const int n_tiles8 = rv_cdiv(d->w_out, CONV_TW) * rv_cdiv(d->h_out, 8);
    const bool nw8 = tiles == 4 && !f32 && !p->gather && !knobs.no_nw8 && (one_wg || n_tiles8 <= 2048);
    if (p->gather) {                                   // only the fp16 strided predictors need it
        RV_CHECK(!f32 && !hi1, "conv: gather mode is built for the fp16 hi+lo path only");
        return 0;
    }
    if (hi1) {                                         // SPyNet's streamed 7x7 convs (Engine.flow): half the weight stream, half the MFMAs
        RV_CHECK(MT <= 2, "conv: single-fp16 weights are built for the streamed stride-1 convs (MT=%d)", MT);
        if (nw8) { p->TILES = 2; p->NW = 8; }
        return 0;
    }
    // lean epilogue: fp16 HWC output, slopes in [0, 1], maps addressable with 32-bit element offsets, tile coordinates in
    // the packed chunk descriptor's range
    const int max_c = d->out_c > d->mul_c ? (d->out_c > d->res_c ? d->out_c : d->res_c) : (d->mul_c > d->res_c ? d->mul_c : d->res_c);
    const bool lean = resident && !f32 && !knobs.no_lean_epi && d->out_mode == REFVSR_OUT_NHWC16 && d->act_slope >= 0.f && d->act_slope <= 1.f &&
                      d->post_slope >= 0.f && d->post_slope <= 1.f && (long long)d->h_out * d->w_out * (long long)max_c < (1ll << 31);
    p->EPI = lean ? 1 : 0;
    if (w16) { p->TILES = 2; p->NW = 16; }
    else if (nw8) { p->TILES = 2; p->NW = 8; }
    // the exact-fp32 convs (VGG head of the matching) on 4 x 32 tiles: eight waves with one pixel group each (fp32 MFMAs are
    // slow enough that the lost fragment reuse costs nothing: 64->64 at 270p 115 -> 105 us)
    else if (!knobs.no_nw8 && f32 && tiles == 2 && (MT == 1 || MT == 2)) { p->TILES = 1; p->NW = 8; }
    return 0;
}
