// Prints what csrc/cnn_plan.h decides, in the vocabulary of tests/cnn_layer_ref.py (plan), for
// tests/test_cnn_layer_ref_host.py.  Host C++17, nothing but the header: c++ -std=c++17 -I csrc cnn_plan_dump.cpp.
//
// stdout: the constants and configuration tables, one "NAME values" line each, a line "---", then one line per query read
// from stdin.
//   "forms dtype i cin cout pool"  ->  the capability record: bf16_rows ktot gemm frag_bf16 frag_x3 first_x3
//   "dtype n_layers (cin cout pool)... H W mode" (dtype fp32 | bf16x3 | bf16_approx; mode forward | conv_output)  ->
//       "none" when the image vanishes inside the network, else the fields below joined by " | ":
//       per layer: kernel nt band n_bands lds=<dynamic LDS of the launch> grid=<x per clip>,<y> fused odd_hw <in>-><out>
//       buf=<one ping-pong buffer for 1 clip>,<for 3 clips> head_hw=<the tail kernel's HW>
//       (single bf16, refused) unsupported=<layer> <its input image>
#include <cstdio>
#include <cstring>

#include "cnn_plan.h"

using namespace cough;

// the vocabulary of tests/cnn_layer_ref.py (plan)
static const char* plan_name(const CnnLayerPlan& s) {
    switch (s.kernel) {
        case CNN_FIRST: return "first";
        case CNN_FIRST_X3: return "first_x3";
        case CNN_CONV_F32: return "conv_f32";
        case CNN_LDS_X3: return "lds_x3";
        case CNN_LDS_BF16: return s.band >= 1 ? "lds_bf16" : "unsupported";
        case CNN_GEMM_BF16: return "gemm_bf16";
        case CNN_CONV_BF16: return "conv_bf16";
    }
    return "?";
}

static int dtype_of(const char* dt) {
    return !std::strcmp(dt, "fp32") ? PLAN_FP32 : !std::strcmp(dt, "bf16x3") ? PLAN_BF16X3 : !std::strcmp(dt, "bf16_approx") ? PLAN_BF16 : -1;
}

int main() {
    std::printf("CNN_FIRST_MAXL %d\nCNN_FIRST_LDS_LIMIT %zu\nCNN_LDS_UNP %d\n", CNN_FIRST_MAXL, CNN_FIRST_LDS_LIMIT, CNN_LDS_UNP);
    std::printf("CNN_LDS_CFG");
    for (const LdsCfg& c : CNN_LDS_CFG) std::printf(" %d %d %d", c.cin, c.nt, c.mw);
    std::printf("\nCNN_X3_TABLE");
    for (const X3Cfg& c : CNN_X3_TABLE) std::printf(" %d %d %d %d %d %d %d", c.cin, c.nt, c.mw, c.wm, c.wn, c.pieces, int(c.lean));
    std::printf("\nCNN_X3_THREADS");
    for (const X3Cfg& c : CNN_X3_TABLE) std::printf(" %d", x3_threads(c));
    std::printf("\nCNN_X3_MAX_LDS");
    for (const X3Cfg& c : CNN_X3_TABLE) std::printf(" %d", x3_max_lds(c));
    std::printf("\nPLAN_MAX_LAYERS %d\n---\n", PLAN_MAX_LAYERS);

    char dt[32], mode[32], line[8192];
    while (std::scanf("%31s", dt) == 1) {
        if (!std::strcmp(dt, "forms")) {
            int i, cin, cout, pool;
            if (std::scanf("%31s %d %d %d %d", dt, &i, &cin, &cout, &pool) != 5 || dtype_of(dt) < 0) {
                std::fprintf(stderr, "bad forms query\n");
                return 2;
            }
            const LayerForms f = layer_forms(dtype_of(dt), i, cin, cout, pool);
            std::printf("%d %d %d %d %d %d\n", int(f.bf16_rows), f.ktot, int(f.gemm), int(f.frag_bf16), int(f.frag_x3), int(f.first_x3));
            continue;
        }
        CnnDims dims[PLAN_MAX_LAYERS];
        int nl, H, W;
        bool good = dtype_of(dt) >= 0 && std::scanf("%d", &nl) == 1 && nl >= 1 && nl <= PLAN_MAX_LAYERS;
        for (int i = 0; good && i < nl; ++i) good = std::scanf("%d %d %d", &dims[i].cin, &dims[i].cout, &dims[i].pool) == 3;
        good = good && std::scanf("%d %d %31s", &H, &W, mode) == 3 && (!std::strcmp(mode, "forward") || !std::strcmp(mode, "conv_output"));
        if (!good) {
            std::fprintf(stderr, "bad query: %s ...\n", dt);
            return 2;
        }
        const bool fwd = !std::strcmp(mode, "forward");
        const CnnPlan p = plan_cnn(dtype_of(dt), dims, nl, H, W, fwd, fwd ? -1 : nl - 1);
        if (!p.ok) {
            std::puts("none");
            continue;
        }
        char* o = line;
        for (int i = 0; i < p.n_layers; ++i) {
            const CnnLayerPlan& s = p.layer[i];
            o += std::sprintf(o, "%s %d %d %d lds=%zu grid=%d,%d %d %d %dx%d->%dx%d | ", plan_name(s), s.nt, s.band, s.n_bands, s.lds, s.gx,
                              s.gy, int(s.fused_mean), int(s.kernel == CNN_FIRST_X3 && s.in.h * s.in.w % 2 == 1), s.in.h, s.in.w,
                              s.out.h, s.out.w);
        }
        o += std::sprintf(o, "buf=%zu,%zu head_hw=%d", p.buf_bytes(1), p.buf_bytes(3), p.head_hw);
        if (p.unsupported_layer >= 0) {
            const HW in = p.layer[p.unsupported_layer].in;
            o += std::sprintf(o, " | unsupported=%d %dx%d", p.unsupported_layer, in.h, in.w);
        }
        std::puts(line);
    }
    return 0;
}
