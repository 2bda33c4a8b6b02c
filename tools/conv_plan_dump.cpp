// Prints the launch plans of the generic MFMA convolution (refvsr_amd/csrc/conv_plan.h) and of the fixed-channel kernels
// (refvsr_amd/csrc/fixed_plan.h) for rows of a cases file: a stand-alone host program, no HIP, no GPU.  tests/test_conv_plan.py and
// tests/test_fixed_plan.py pin the plans with it.
//
//   conv_plan_dump CASES             one line per row of CASES: the ConvPlan as key=value tokens, or `rejected: <message>`
//   conv_plan_dump --variants        one line per entry of RV_CONV_VARIANTS
//   conv_plan_dump --fixed CASES     one line per row of CASES: the C24Plan / Rb24Plan as key=value tokens, or `rejected: <message>`
//   conv_plan_dump --fixed-variants  one line per entry of RV_C24_VARIANTS, then of RV_RB24_VARIANTS, each with its key
//
// A row is a line of key=value tokens; `#` starts a comment.  Lower-case keys are RefvsrConv fields (mt = mt_per_block, act / post =
// the slopes; src1 / mul / res / res_planar = 0 | 1: pointer present; ksteps omitted = what the geometry gives; h_in / w_in omitted =
// stride times the output size), upper-case keys the knobs of ConvKnobs by the suffix of their environment variable (RES_MAX=12,
// NO_NW8=1, ...).  Fields not named keep the defaults below.
//
// A --fixed row names its entry point with op = conv24 | conv32 | conv48 (c0, c1) | shuffle2 | conv_last (c) | conf_alpha (cout, up; h x w
// = the confidence maps) | rb24 (the resblock24 chain: slope = act_slope) | hr_last (refvsr_conv_hr_last); wf = 1: the `_f16w` twin,
// mm = 1: the `_batch` entry with `batch` maps; h, w; CONV48_WAVES = the value of REFVSR_CONV48_WAVES (0: unset); waves / store / probe
// = the resblock24 knobs (refvsr_set_resblock24_waves / _store, a probe buffer set), cus = the CU budget of the stream.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../refvsr_amd/csrc/conv_plan.h"
#include "../refvsr_amd/csrc/fixed_plan.h"

static char g_error[512];
void refvsr_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

static void print_variant(int MT, int TILES, bool F32, bool GATHER, bool RESIDENT, int EPI, int NW, bool HI1) {
    printf("MT=%d TILES=%d F32=%d GATHER=%d RESIDENT=%d EPI=%d NW=%d HI1=%d", MT, TILES, (int)F32, (int)GATHER, (int)RESIDENT, EPI, NW, (int)HI1);
}

static int dump_row(const std::string& line) {
    static int dummy;                                  // what the present pointers point at (a plan reads no memory)
    RefvsrConv d;
    memset(&d, 0, sizeof(d));
    ConvKnobs k;
    d.src0 = d.wpack = d.out = &dummy;
    d.bias = reinterpret_cast<const float*>(&dummy);
    d.c0 = 24; d.h_in = d.w_in = -1; d.h_out = 16; d.w_out = 24;
    d.ksize = 3; d.stride = 1; d.pad = 1; d.cout = 48; d.mt_per_block = 2; d.ksteps = -1;
    d.act_slope = d.post_slope = 1.0f; d.out_c = 48;
    int src1 = -1;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "conv_plan_dump: token without '=': %s\n", tok.c_str()); return 1; }
        const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
        const long long n = atoll(val.c_str());
        const void* ptr = n ? &dummy : nullptr;
        if (key == "c0") d.c0 = (int)n;
        else if (key == "c1") d.c1 = (int)n;
        else if (key == "src0") d.src0 = ptr;
        else if (key == "src1") src1 = (int)n;
        else if (key == "h_in") d.h_in = (int)n;
        else if (key == "w_in") d.w_in = (int)n;
        else if (key == "h_out") d.h_out = (int)n;
        else if (key == "w_out") d.w_out = (int)n;
        else if (key == "ksize") d.ksize = (int)n;
        else if (key == "stride") d.stride = (int)n;
        else if (key == "pad") d.pad = (int)n;
        else if (key == "cout") d.cout = (int)n;
        else if (key == "mt") d.mt_per_block = (int)n;
        else if (key == "ksteps") d.ksteps = (int)n;
        else if (key == "act") d.act_slope = (float)atof(val.c_str());
        else if (key == "post") d.post_slope = (float)atof(val.c_str());
        else if (key == "mul") d.mul = ptr;
        else if (key == "mul_c") d.mul_c = (int)n;
        else if (key == "res") d.res = ptr;
        else if (key == "res_c") d.res_c = (int)n;
        else if (key == "out_mode") d.out_mode = (int)n;
        else if (key == "out_c") d.out_c = (int)n;
        else if (key == "res_planar") d.res_planar = reinterpret_cast<const float*>(ptr);
        else if (key == "f32") d.f32 = (int)n;
        else if (key == "batch") d.batch = (int)n;
        else if (key == "bs_src0") d.bs_src0 = (size_t)n;
        else if (key == "bs_src1") d.bs_src1 = (size_t)n;
        else if (key == "bs_out") d.bs_out = (size_t)n;
        else if (key == "bs_res_planar") d.bs_res_planar = (size_t)n;
        else if (key == "NO_PERSIST") k.no_persist = n != 0;
        else if (key == "RES_MAX") k.res_max = (int)n;
        else if (key == "TILES") k.tiles = (int)n;
        else if (key == "NO_W16") k.no_w16 = n != 0;
        else if (key == "RING") k.ring = (int)n;
        else if (key == "NO_NW8") k.no_nw8 = n != 0;
        else if (key == "NO_PREFETCH") k.no_prefetch = n != 0;
        else if (key == "NO_LEAN_EPI") k.no_lean_epi = n != 0;
        else { fprintf(stderr, "conv_plan_dump: unknown key %s\n", key.c_str()); return 1; }
    }
    if (src1 < 0 ? d.c1 > 0 : src1 > 0) d.src1 = &dummy;
    if (d.h_in < 0) d.h_in = d.h_out * d.stride;
    if (d.w_in < 0) d.w_in = d.w_out * d.stride;
    if (d.ksteps < 0 && d.ksize >= 1 && d.ksize <= 7 && d.c0 > 0 && d.c1 >= 0) d.ksteps = rv_ksteps(d.ksize, (d.c0 + d.c1) / (d.f32 == 1 ? 4 : 8));
    ConvPlan p;
    g_error[0] = 0;
    if (conv_plan(&d, k, &p)) {
        printf("rejected: %s\n", g_error);
        return 0;
    }
    print_variant(p.MT, p.TILES, p.F32, p.GATHER, p.RESIDENT, p.EPI, p.NW, p.HI1);
    printf(" nz=%d lds=%zu tab_bytes=%d wl_bytes=%d ring=%d LH=%d LW=%d ps=%d G=%d S=%d tiles_x=%d n_xy=%d gather=%d prefetch=%d\n", p.nz, p.lds,
           p.tab_bytes, p.wl_bytes, p.ring, p.LH, p.LW, p.ps, p.G, p.S, p.tiles_x, p.n_xy, p.gather, p.prefetch);
    return 0;
}

static void print_c24_variant(int COUT, int NCG0, int NCG1, int NWV, int TH, int WPS, int SHUF, int CONF, int HALF, int MM, int WF) {
    printf("COUT=%d NCG0=%d NCG1=%d NWV=%d TH=%d WPS=%d SHUF=%d CONF=%d HALF=%d MM=%d WF=%d", COUT, NCG0, NCG1, NWV, TH, WPS, SHUF, CONF, HALF, MM, WF);
}
static void print_rb24_variant(bool RELU, int NWV, bool PROBE, int TH, int STORE, int HEAD, int WF) {
    printf("RELU=%d NWV=%d PROBE=%d TH=%d STORE=%d HEAD=%d WF=%d", (int)RELU, NWV, (int)PROBE, TH, STORE, HEAD, WF);
}

static int dump_fixed_row(const std::string& line) {
    std::string op = "conv24";
    int c0 = 24, c1 = 0, c = 24, cout = 24, up = 1, wf = 0, mm = 0, batch = 1, h = 270, w = 480, cus = 256;
    float slope = 0.f;
    C24Knobs ck;
    Rb24Knobs rk;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "conv_plan_dump: token without '=': %s\n", tok.c_str()); return 1; }
        const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
        const int n = atoi(val.c_str());
        if (key == "op") op = val;
        else if (key == "c0") c0 = n;
        else if (key == "c1") c1 = n;
        else if (key == "c") c = n;
        else if (key == "cout") cout = n;
        else if (key == "up") up = n;
        else if (key == "wf") wf = n;
        else if (key == "mm") mm = n;
        else if (key == "batch") batch = n;
        else if (key == "h") h = n;
        else if (key == "w") w = n;
        else if (key == "CONV48_WAVES") ck.conv48_w8 = n == 8;
        else if (key == "slope") slope = (float)atof(val.c_str());
        else if (key == "waves") rk.waves = n;
        else if (key == "store") rk.store = n;
        else if (key == "probe") rk.probe = n != 0;
        else if (key == "cus") cus = n;
        else { fprintf(stderr, "conv_plan_dump: unknown key %s\n", key.c_str()); return 1; }
    }
    if (!mm) batch = 1;                                // a single-map entry has no batch argument
    g_error[0] = 0;
    if (op == "rb24" || op == "hr_last") {
        Rb24Plan p;
        if (rb24_plan(op == "hr_last", wf, slope == 0.f, h, w, batch, cus, rk, &p)) { printf("rejected: %s\n", g_error); return 0; }
        print_rb24_variant(p.RELU, p.NWV, p.PROBE, p.TH, p.STORE, p.HEAD, p.WF);
        printf(" lds=%d tiles_x=%d tpm=%d n_tiles=%d\n", p.lds, p.tiles_x, p.tpm, p.n_tiles);
        return 0;
    }
    C24Plan p;
    int rc;
    if (op == "conv24") rc = c24_plan(C24_CONV24, c0, c1, mm, wf, batch, h, w, ck, &p);
    else if (op == "conv32") rc = c24_plan(C24_CONV32, c0, c1, 0, wf, 1, h, w, ck, &p);
    else if (op == "conv48") rc = c24_plan(C24_CONV48, c0, c1, 0, 0, 1, h, w, ck, &p);
    else if (op == "shuffle2") rc = c24_plan(C24_SHUFFLE2, c, 0, mm, wf, batch, h, w, ck, &p);
    else if (op == "conf_alpha") rc = c24_plan(C24_CONF_ALPHA, cout, up, mm, wf, batch, h, w, ck, &p);
    else if (op == "conv_last") rc = c24_plan(C24_CONV_LAST, c, 0, 0, 0, 1, h, w, ck, &p);
    else { fprintf(stderr, "conv_plan_dump: unknown op %s\n", op.c_str()); return 1; }
    if (rc || p.no_twin) { printf("rejected: %s\n", rc ? g_error : p.no_twin); return 0; }
    print_c24_variant(p.COUT, p.NCG0, p.NCG1, p.NWV, p.TH, p.WPS, p.SHUF, p.CONF, p.HALF, p.MM, p.WF);
    printf(" nz=%d lds=%d tiles_x=%d tpm=%d n_tiles=%d\n", p.nz, p.lds, p.tiles_x, p.tpm, p.n_tiles);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--fixed-variants")) {
#define RV_PRINT_VARIANT(...) print_c24_variant(__VA_ARGS__); printf(" key=%lld\n", c24_variant_key(__VA_ARGS__));
        RV_C24_VARIANTS(RV_PRINT_VARIANT)
#undef RV_PRINT_VARIANT
#define RV_PRINT_VARIANT(...) print_rb24_variant(__VA_ARGS__); printf(" key=%d\n", rb24_variant_key(__VA_ARGS__));
        RV_RB24_VARIANTS(RV_PRINT_VARIANT)
#undef RV_PRINT_VARIANT
        return 0;
    }
    const bool fixed = argc == 3 && !strcmp(argv[1], "--fixed");
    if (fixed) { argv[1] = argv[2]; argc = 2; }
    if (argc == 2 && !strcmp(argv[1], "--variants")) {
#define RV_PRINT_VARIANT(...) print_variant(__VA_ARGS__); printf(" key=%d\n", conv_variant_key(__VA_ARGS__));
        RV_CONV_VARIANTS(RV_PRINT_VARIANT)
#undef RV_PRINT_VARIANT
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: conv_plan_dump CASES | --variants | --fixed CASES | --fixed-variants\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { fprintf(stderr, "conv_plan_dump: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(f, line)) {
        line = line.substr(0, line.find('#'));
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        if (fixed ? dump_fixed_row(line) : dump_row(line)) return 2;
    }
    return 0;
}
