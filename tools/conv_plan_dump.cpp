// Prints the launch plan of the generic MFMA convolution (refvsr_amd/csrc/conv_plan.h) for descriptor rows: a stand-alone host
// program, no HIP, no GPU.  tests/test_conv_plan.py pins the plans with it.
//
//   conv_plan_dump CASES      one line per row of CASES: the ConvPlan as key=value tokens, or `rejected: <message>`
//   conv_plan_dump --variants one line per entry of RV_CONV_VARIANTS
//
// A row is a line of key=value tokens; `#` starts a comment.  Lower-case keys are RefvsrConv fields (mt = mt_per_block, act / post =
// the slopes; src1 / mul / res / res_planar = 0 | 1: pointer present; ksteps omitted = what the geometry gives; h_in / w_in omitted =
// stride times the output size), upper-case keys the knobs of ConvKnobs by the suffix of their environment variable (RES_MAX=12,
// NO_NW8=1, ...).  Fields not named keep the defaults below.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../refvsr_amd/csrc/conv_plan.h"

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

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--variants")) {
#define RV_PRINT_VARIANT(...) print_variant(__VA_ARGS__); printf(" key=%d\n", conv_variant_key(__VA_ARGS__));
        RV_CONV_VARIANTS(RV_PRINT_VARIANT)
#undef RV_PRINT_VARIANT
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: conv_plan_dump CASES | --variants\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { fprintf(stderr, "conv_plan_dump: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(f, line)) {
        line = line.substr(0, line.find('#'));
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        if (dump_row(line)) return 2;
    }
    return 0;
}
