// Launch plans of the fixed-channel kernels (conv24.hip: conv24_kernel; resblock24.hip: resblock24_kernel): the shape-support checks
// and the choice of the instantiation, with its row groups, LDS bytes and tile counts, as pure functions of the op, its shape
// arguments and the A/B knobs.  Also the ONE copy of the blob and LDS byte counts of both kernels.  No HIP call, no HIP header: it
// also compiles with a plain host compiler, which is how tests/test_fixed_plan.py pins it (tools/conv_plan_dump.cpp).  What depends
// on the device -- the grid cap of the persistent kernels -- stays with the launchers; the CU budget of the stream is an input.
#pragma once
#include <stdlib.h>

#include "../../include/refvsr_hip.h"
#include "plan_common.h"
#include "conv24_plan.h"

#ifndef REFVSR_RB24_STORE_DEFAULT
#define REFVSR_RB24_STORE_DEFAULT 1
#endif

// Every instantiation of conv24_kernel, X(COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF): the ONLY place where they are
// written down.  conv24.hip expands the list into its dispatch (a switch on the key: a list entry twice is a compile error), host-only
// code into the list of keys.
#define RV_C24_VARIANTS(X)                                                                                                        \
    /* 24 outputs: 24 | 16 | 8 + 24 | 24 + 24 inputs; single-map, fp16 weights, multi-map, both */                               \
    RV_C24_VARIANTS24(X, 0, 0) RV_C24_VARIANTS24(X, 0, 1) RV_C24_VARIANTS24(X, 1, 0) RV_C24_VARIANTS24(X, 1, 1)                   \
    /* 32 outputs: 32 | 8 inputs */                                                                                               \
    X(32, 4, 0, 8, 8, 4, 0, 0, 0, 0, 0) X(32, 1, 0, 8, 8, 4, 0, 0, 0, 0, 0)                                                       \
    X(32, 4, 0, 8, 8, 4, 0, 0, 0, 0, 1) X(32, 1, 0, 8, 8, 4, 0, 0, 0, 0, 1)                                                       \
    /* 48 outputs: 48 + 48 (two channel halves) | 8 + 48 | 48 on 8 waves | 48 on 16 waves | 16 inputs */                          \
    X(24, 6, 6, 16, 8, 4, 0, 0, 1, 0, 0) X(48, 1, 6, 16, 8, 4, 0, 0, 0, 0, 0)                                                     \
    X(48, 6, 0, 8, 16, 2, 0, 0, 0, 0, 0) X(48, 6, 0, 16, 16, 4, 0, 0, 0, 0, 0) X(48, 2, 0, 8, 8, 4, 0, 0, 0, 0, 0)                \
    /* pixel shuffle: C = 24, C = 48, C = 24 with fp16 weights | multi-map | both */                                              \
    X(48, 3, 0, 8, 8, 4, 24, 0, 0, 0, 0) X(48, 6, 0, 16, 16, 4, 48, 0, 0, 0, 0)                                                   \
    X(48, 3, 0, 8, 8, 4, 24, 0, 0, 0, 1) X(48, 3, 0, 8, 8, 4, 24, 0, 0, 1, 0) X(48, 3, 0, 8, 8, 4, 24, 0, 0, 1, 1)                \
    /* confidence fusion, up = 1 | 2: 24 outputs, 48 outputs, 24 outputs with fp16 weights | multi-map | both */                  \
    X(24, 2, 0, 8, 8, 4, 0, 1, 0, 0, 0) X(24, 2, 0, 8, 8, 4, 0, 2, 0, 0, 0)                                                       \
    X(48, 2, 0, 8, 8, 4, 0, 1, 0, 0, 0) X(48, 2, 0, 8, 8, 4, 0, 2, 0, 0, 0)                                                       \
    X(24, 2, 0, 8, 8, 4, 0, 1, 0, 0, 1) X(24, 2, 0, 8, 8, 4, 0, 2, 0, 0, 1)                                                       \
    X(24, 2, 0, 8, 8, 4, 0, 1, 0, 1, 0) X(24, 2, 0, 8, 8, 4, 0, 2, 0, 1, 0)                                                       \
    X(24, 2, 0, 8, 8, 4, 0, 1, 0, 1, 1) X(24, 2, 0, 8, 8, 4, 0, 2, 0, 1, 1)                                                       \
    /* output head: 24 | 48 inputs */                                                                                             \
    X(3, 3, 0, 8, 8, 4, 0, 0, 0, 0, 0) X(3, 6, 0, 8, 8, 4, 0, 0, 0, 0, 0)
#define RV_C24_VARIANTS24(X, MM, WF)                                                                                              \
    X(24, 3, 0, 8, 8, 4, 0, 0, 0, MM, WF) X(24, 2, 0, 8, 8, 4, 0, 0, 0, MM, WF) X(24, 1, 3, 8, 8, 4, 0, 0, 0, MM, WF)             \
    X(24, 3, 3, 8, 8, 4, 0, 0, 0, MM, WF)

// Every instantiation of resblock24_kernel, X(RELU, NWV, PROBE, TH, STORE, HEAD, WF): 2 probe, then per weight format 2 four-wave
// and 8 plain blocks, then 2 output heads
#define RV_RB24_VARIANTS(X)                                                                                                       \
    X(true, 8, true, 8, 0, 0, 0) X(true, 16, true, 16, 0, 0, 0)                                                                   \
    RV_RB24_VARIANTS_WF(X, 0) RV_RB24_VARIANTS_WF(X, 1)                                                                           \
    X(false, 16, false, 16, 0, 1, 0) X(false, 8, false, 8, 0, 1, 0)
#define RV_RB24_VARIANTS_WF(X, WF)                                                                                                \
    X(true, 4, false, 8, 0, 0, WF) X(false, 4, false, 8, 0, 0, WF)                                                                \
    X(true, 16, false, 16, 1, 0, WF) X(true, 16, false, 16, 0, 0, WF) X(true, 8, false, 8, 1, 0, WF) X(true, 8, false, 8, 0, 0, WF) \
    X(false, 16, false, 16, 1, 0, WF) X(false, 16, false, 16, 0, 0, WF) X(false, 8, false, 8, 1, 0, WF) X(false, 8, false, 8, 0, 0, WF)

// the template arguments packed into one integer: what a plan is looked up by
constexpr long long c24_variant_key(int COUT, int NCG0, int NCG1, int NWV, int TH, int WPS, int SHUF, int CONF, int HALF, int MM, int WF) {
    return COUT | NCG0 << 6 | NCG1 << 10 | NWV << 14 | TH << 19 | WPS << 24 | (long long)SHUF << 27 | (long long)CONF << 33 | (long long)HALF << 35 |
           (long long)MM << 36 | (long long)WF << 37;
}
constexpr int rb24_variant_key(bool RELU, int NWV, bool PROBE, int TH, int STORE, int HEAD, int WF) {
    return (int)RELU | NWV << 1 | (int)PROBE << 6 | TH << 7 | STORE << 12 | HEAD << 13 | WF << 14;
}

namespace {
// ---- conv24_kernel: bytes ----------------------------------------------------------------------------------------------------------
// Fragments per K-step.  Weight format WF = 0: hi + lo (COUT = 24: [hi 0-15] [lo 0-15] [hi 16-23 | lo 16-23]; 32 | 48: [hi | lo] per
// 16 channels; 3: rows 0-2 hi, rows 8-10 lo).  WF = 1 (ABI 15, config.weight_precision = 'fp16'): plain fp16 weights, one fragment
// per 16 output channels -- 24: [rows 0-15] [rows 16-23 + 8 zero rows]; 32 | 48: [rows 16 m ..] -- no lo term, no fold.
constexpr int c24_nf(int cout, int wf) { return wf ? (cout == 24 ? 2 : cout / 16) : cout == 24 ? 3 : cout == 3 ? 1 : cout / 8; }
// one parameter blob: [K-steps x fragments x 1 KiB][bias tail]; ncg = 16-byte channel groups of both sources
constexpr int c24_blob_bytes(int cout, int ncg, int wf) { return c24_steps(ncg) * c24_nf(cout, wf) * 1024 + (cout == 48 ? 256 : 128); }
// row groups (blockIdx.y, one blob each) of the pixel-shuffle / channel-half variants
constexpr int c24_nz(int shuf, int half) { return half ? 2 : shuf == 0 ? 1 : shuf == 24 ? 2 : 4; }
// dynamic LDS: [blob][x tile: (TH + 2) x 34 pixels x (ncg | 1) slots][CONF: pair tile, first conv's weights and bias]
constexpr int c24_lds(int cout, int ncg, int th, int conf, int wf) {
    return c24_blob_bytes(cout, ncg, wf) + (th + 2) * C24_XW * (ncg | 1) * 16 + (conf ? 2 * (th + 4) * (C24_XW + 2) * 4 + 18 * 16 * 4 + 64 : 0);
}

// ---- resblock24_kernel: tile constants and bytes --------------------------------------------------------------------------------------
constexpr int RB_TW = 32;                                 // tile width; the tile height TH is a template parameter (8 | 16)
constexpr int RB_XW = RB_TW + 4;                          // x tile: (TH + 4) x 36 pixels
constexpr int RB_IW = RB_TW + 2;                          // intermediate: (TH + 2) x 34
constexpr int RB_PXB = 48;                                // bytes per pixel (24 halfs)
constexpr int RB_ROWB = RB_XW * RB_PXB;                   // 1728 bytes per tile row
constexpr int RB_RCH = RB_ROWB / 16;                      // 108 chunks per tile row
constexpr int rb_xbytes(int th) { return (th + 4) * RB_ROWB; }         // 20736 (TH = 8) | 34560 (TH = 16)
constexpr int RB_S = 7, RB_NF = 3;
constexpr int RB_WB = RB_S * RB_NF * 1024;                // 21504 bytes of fragments per conv
constexpr int RB_BIAS = 2 * RB_WB;                        // 43008
constexpr int RB_BLOB = RB_BIAS + 256;                    // 43264
constexpr int RB_XT = RB_BLOB;                            // LDS offset of the x tile
static_assert(RB_BLOB == REFVSR_RESBLOCK24_BLOB_BYTES, "blob size is part of the C-ABI");
// Weight format WF (ABI 15): 0 = hi + lo in three fragments per K-step; 1 = plain fp16 weights in TWO fragments per K-step,
// [rows 0-15] [rows 16-23 + 8 zero rows] -- no lo term, no fold (config.weight_precision = 'fp16', packing.py:pack_resblock24_f16w)
constexpr int rb_nf(int wf) { return wf ? 2 : RB_NF; }
constexpr int rb_wb(int wf) { return RB_S * rb_nf(wf) * 1024; }      // 21504 | 14336
constexpr int rb_bias(int wf) { return 2 * rb_wb(wf); }
constexpr int rb_blob(int wf) { return rb_bias(wf) + 256; }          // 43264 | 28928
// 64000 (TH = 8: two workgroups per CU) | 77824 (TH = 16: one); WF = 1: 49664 | 63488
constexpr int rb_lds_wf(int th, int wf) { return rb_blob(wf) + rb_xbytes(th); }
static_assert(rb_blob(1) == REFVSR_RESBLOCK24_F16W_BLOB_BYTES, "blob size is part of the C-ABI");
}  // namespace

// ---- conv24_kernel: the plan ---------------------------------------------------------------------------------------------------------
// the ops of conv24.hip and their shape arguments (x0, x1)
// (the values are public: refvsr_conv24_variant takes them)
enum C24Op {
    C24_CONV24 = REFVSR_C24_CONV24,            // refvsr_conv24*: (c0, c1) input channels of the two sources
    C24_CONV32 = REFVSR_C24_CONV32,            // refvsr_conv32*: (c0, c1)
    C24_CONV48 = REFVSR_C24_CONV48,            // refvsr_conv48: (c0, c1)
    C24_SHUFFLE2 = REFVSR_C24_SHUFFLE2,        // refvsr_conv_shuffle2*: (c, -)
    C24_CONF_ALPHA = REFVSR_C24_CONF_ALPHA,    // refvsr_conf_alpha*: (cout, up); h x w = the confidence maps, the conv runs on the (up h) x (up w) grid
    C24_CONV_LAST = REFVSR_C24_CONV_LAST,      // refvsr_conv_last*: (c, -)
};
constexpr bool c24_supported(C24Op op, int x0, int x1) {
    return op == C24_CONV24   ? (x0 == 24 && x1 == 0) || (x0 == 16 && x1 == 0) || (x0 == 8 && x1 == 24) || (x0 == 24 && x1 == 24)
           : op == C24_CONV32 ? (x0 == 32 && x1 == 0) || (x0 == 8 && x1 == 0)
           : op == C24_CONV48 ? (x0 == 48 && x1 == 0) || (x0 == 16 && x1 == 0) || (x0 == 48 && x1 == 48) || (x0 == 8 && x1 == 48)
                              : x0 == 24 || x0 == 48;      // pixel shuffle, output head (C24_CONF_ALPHA: c24_plan checks cout and up apart)
}

// A/B knob of the fixed-channel convs (README: REFVSR_CONV48_WAVES); the default is the shipped behaviour
struct C24Knobs {
    bool conv48_w8 = false;          // REFVSR_CONV48_WAVES=8: the 48 -> 48 conv on eight waves with four pixel groups each (default: sixteen with two)
};
static inline C24Knobs c24_knobs_from_env() {
    C24Knobs k;
    const char* v = getenv("REFVSR_CONV48_WAVES");
    k.conv48_w8 = v && atoi(v) == 8;
    return k;
}

struct C24Plan {
    int COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF;   // the instantiation
    int nz;                          // gridDim.y: row groups
    int lds;                         // dynamic LDS bytes
    int tiles_x, tpm, n_tiles;       // TH x 32 tiles per row / per map / per launch
    const char* no_twin;             // set: the shape is supported but has no kernel in this weight format -- no instantiation above;
                                     // reported where the dispatch finds no kernel, behind the argument checks
    long long key() const { return c24_variant_key(COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF); }
};

// 0 and *p filled, or 1 and the message set (refvsr_set_error).  mm: the `_batch` entry (batch maps per launch), wf: the `_f16w` twin
static int c24_plan(C24Op op, int x0, int x1, int mm, int wf, int batch, int h, int w, const C24Knobs& knobs, C24Plan* p) {
    *p = C24Plan();
    int cout = 24, ncg0 = x0 / 8, ncg1 = 0, nwv = 8, th = 8, wps = 4, shuf = 0, conf = 0, half = 0;
    switch (op) {
    case C24_CONV24: {
        const char* who = mm ? "conv24_batch" : "conv24";
        RV_CHECK(c24_supported(op, x0, x1), "%s: %d + %d input channels not supported", who, x0, x1);
        RV_CHECK(batch >= 1 && batch <= REFVSR_MAX_MAPS, "%s: 1..%d maps per launch", who, REFVSR_MAX_MAPS);
        ncg1 = x1 / 8;
        break;
    }
    case C24_CONV32:
        RV_CHECK(c24_supported(op, x0, x1), "conv32: %d + %d input channels not supported", x0, x1);
        cout = 32;
        break;
    case C24_CONV48:
        RV_CHECK(c24_supported(op, x0, x1), "conv48: %d + %d input channels not supported", x0, x1);
        cout = 48; ncg1 = x1 / 8;
        // 84 KB of weights + 18 x 34-pixel tile: one workgroup per CU.  Sixteen waves with two pixel groups each (default), or eight
        // waves with four (37 % fewer LDS fragment reads, half the waves per SIMD)
        if (x0 == 48 && x1 == 0) { th = 16; nwv = knobs.conv48_w8 ? 8 : 16; wps = knobs.conv48_w8 ? 2 : 4; }
        // 48 + 48: two channel halves of 24 on blockIdx.y.  8 + 48 -> 48, the input conv of ResidualBlocksWithInputConv on
        // cat([lr, feat]) (RefVSR.py:340-343): NCG = 7 plan, 108 KB of weights resident next to the 38 KB tile.  Sixteen waves with
        // one pixel group each
        if (x1 == 48) { nwv = 16; if (x0 == 48) { cout = 24; half = 1; } }
        break;
    case C24_SHUFFLE2: {
        const char* who = mm ? "conv_shuffle2_batch" : "conv_shuffle2";
        if (mm) RV_CHECK(x0 == 24, "conv_shuffle2_batch: %d channels not supported (24)", x0);
        RV_CHECK(c24_supported(op, x0, x1), "conv_shuffle2: %d channels not supported", x0);
        RV_CHECK(batch >= 1 && batch <= REFVSR_MAX_MAPS, "%s: 1..%d maps per launch", who, REFVSR_MAX_MAPS);
        cout = 48; shuf = x0;
        if (x0 == 48) { th = 16; nwv = 16; if (wf) p->no_twin = "conv_shuffle2_f16w: 24 channels only (the mid_channels = 24 family)"; }
        break;
    }
    case C24_CONF_ALPHA: {
        const char* who = mm ? "conf_alpha_batch" : "conf_alpha";
        if (mm) RV_CHECK(batch >= 1 && batch <= REFVSR_MAX_MAPS, "conf_alpha_batch: bad args (1..%d maps)", REFVSR_MAX_MAPS);
        RV_CHECK(x1 == 1 || x1 == 2, "%s: up must be 1 or 2", who);
        if (mm) RV_CHECK(x0 == 24, "conf_alpha_batch: %d output channels not supported (24)", x0);
        else RV_CHECK(x0 == 24 || x0 == 48, "conf_alpha: %d output channels not supported (24 | 48)", x0);
        cout = x0; ncg0 = 2; conf = x1;
        h *= x1; w *= x1;
        if (x0 == 48 && wf) p->no_twin = "conf_alpha_f16w: 24 output channels only (the mid_channels = 24 family)";
        break;
    }
    case C24_CONV_LAST:
        RV_CHECK(c24_supported(op, x0, x1), "conv_last: %d input channels not supported (24 | 48)", x0);
        cout = 3;
        break;
    }
    if (p->no_twin) return 0;
    p->COUT = cout; p->NCG0 = ncg0; p->NCG1 = ncg1; p->NWV = nwv; p->TH = th; p->WPS = wps; p->SHUF = shuf; p->CONF = conf; p->HALF = half;
    p->MM = mm; p->WF = wf;
    p->nz = c24_nz(shuf, half);
    p->lds = c24_lds(cout, ncg0 + ncg1, th, conf, wf);
    p->tiles_x = rv_cdiv(w, C24_TW);
    p->tpm = p->tiles_x * rv_cdiv(h, th);
    p->n_tiles = p->tpm * (mm ? batch : 1);
    return 0;
}

// ---- resblock24_kernel: the plan -----------------------------------------------------------------------------------------------------
// A/B knobs of the fused C = 24 block (refvsr_set_resblock24_store / _waves, refvsr_set_probe); the defaults are the shipped behaviour
struct Rb24Knobs {
    int store = REFVSR_RB24_STORE_DEFAULT;   // 0 | 1: the kernel's STORE parameter
    int waves = 0;                   // 0 = by map size; 4 | 8: 8 x 32 tiles; 16: 16 x 32
    bool probe = false;              // a probe buffer is set: ReLU blocks in the hi + lo format on 8 | 16 waves run the stamping kernels
};

struct Rb24Plan {
    bool RELU; int NWV; bool PROBE; int TH, STORE, HEAD, WF;        // the instantiation
    int lds;                         // dynamic LDS bytes
    int tiles_x, tpm, n_tiles;       // TH x 32 tiles per row / per map / per launch
    int key() const { return rb24_variant_key(RELU, NWV, PROBE, TH, STORE, HEAD, WF); }
};

// head = 0: one fused block over `batch` maps (relu: act_slope == 0); head = 1: the output head (refvsr_conv_hr_last: one map, always leaky).
// cus: the CU budget of the launch's stream.  Returns 0 and *p filled
static int rb24_plan(int head, int wf, bool relu, int h, int w, int batch, int cus, const Rb24Knobs& knobs, Rb24Plan* p) {
    *p = Rb24Plan();
    if (batch < 1 || head) batch = 1;
    // 16 x 32 tiles on sixteen waves (one workgroup per CU: half the weight fill per CU, 10 % less halo work in conv1, 17 % less
    // tile staging) pay on maps of many tiles per workgroup -- 540 x 960: 27.3 -> 26.3 us, 1080 x 1920: 100.1 -> 95.9 us; at
    // 270 x 480 (one tile per workgroup either way) the two shapes are equal (9.3 vs 9.4 us: the fill is latency, not bandwidth,
    // and sixteen waves wait longer at the barriers), below that the 8 x 32 tiles fill more CUs (135 x 240: 6.2 vs 8.2 us)
    const int nt8 = rv_cdiv(w, RB_TW) * rv_cdiv(h, 8) * batch;
    const bool forced = head ? knobs.waves == 8 || knobs.waves == 16 : knobs.waves != 0;   // (the head has no four-wave kernel)
    const int waves = forced ? knobs.waves : (nt8 >= 4 * cus ? 16 : 8);
    p->RELU = !head && relu; p->NWV = waves; p->TH = waves == 16 ? 16 : 8; p->HEAD = head; p->WF = wf;
    p->PROBE = p->RELU && wf == 0 && knobs.probe && waves != 4;                            // tools/probe_resblock24.py
    p->STORE = head || p->PROBE || waves == 4 ? 0 : knobs.store;
    p->lds = rb_lds_wf(p->TH, wf);
    p->tiles_x = rv_cdiv(w, RB_TW);
    p->tpm = p->tiles_x * rv_cdiv(h, p->TH);
    p->n_tiles = p->tpm * batch;
    return 0;
}
