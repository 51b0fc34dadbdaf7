// Prints what csrc/resnet_plan.h decides, in the vocabulary of tests/resnet_layer_ref.py (plan_row, stage_path), for
// tests/test_resnet_layer_ref_host.py.  Host C++17, nothing but the header: c++ -std=c++17 -I csrc resnet_plan_dump.cpp.
//
// stdout: the constants and row lists, one "NAME values" line each, a line "---", then one line per query read from
// stdin.  A query is "dtype channels-kind n_blocks H W" (dtype fp32 | bf16x3 | bf16_approx; kind shipped | generic); its
// line is "none" when the image vanishes inside the network, else the fields below joined by " | ":
//   stem kernel, lds=<dynamic LDS of the launch>
//   per block: kernel body clips stage_path <in>-><out> lds=<bytes the plan sizes>
//   head
//   nan source, by=<block1 | nan_rule_kernel>, a3=<store | skip>
//   (shipped bf16x3 / bf16_approx) pipeline: the last field again for the forward behind the featuriser's fused stem
#include <cstdio>
#include <cstring>

#include "resnet_plan.h"

using namespace cough;

static int put_tail(char* o, const NetPlan& p) {
    return std::sprintf(o, "%s by=%s a3=%s", plan_name(p.nan), p.nan_in_block1 ? "block1" : "nan_rule_kernel",
                        p.store_a3 ? "store" : "skip");
}

int main() {
    std::printf("STEM_SB_MAXL %d\n", STEM_SB_MAXL);
    for (int blk = 0; blk < 2; ++blk) {
        std::printf("RBX_BLOCK%d_ROWS", blk);
        for (int i = 0; i < RBX_NROWS[blk]; ++i) std::printf(" %d", rbx_rows(blk, i));
        std::printf("\n");
    }
    std::printf("RBX_COLS %d %d\n", RBX_COLS[0], RBX_COLS[1]);
    std::printf("RBX_G_TALL %d\n", RBX_G_TALL);
    std::printf("NET_CH %d %d %d\n", NET_CH[0], NET_CH[1], NET_CH[2]);
    std::printf("RB_CFG");
    for (const RbParams& c : RB_CFG) std::printf(" %d %d %d %d %d", c.cin, c.cout, c.g, c.mw, c.waves);
    std::printf("\nRB_FIXED %d %d %d %d\n", RB_FIXED[0].h, RB_FIXED[0].w, RB_FIXED[1].h, RB_FIXED[1].w);
    std::printf("RB_MTMAX %d %d\n", rb_mtmax(RB_CFG[0]), rb_mtmax(RB_CFG[1]));
    std::printf("RB_THREADS %d %d\n", rb_threads(RB_CFG[0]), rb_threads(RB_CFG[1]));
    std::printf("STEM_LDS_LIMIT %zu\nRB_LDS_LIMIT %zu\n", STEM_LDS_LIMIT, RB_LDS_LIMIT);
    std::printf("PLAN_MAX_BLOCKS %d\n---\n", PLAN_MAX_BLOCKS);

    char dt[32], kind[32], line[4096];
    int nb, H, W;
    while (std::scanf("%31s %31s %d %d %d", dt, kind, &nb, &H, &W) == 5) {
        const int dtype = !std::strcmp(dt, "fp32") ? PLAN_FP32 : !std::strcmp(dt, "bf16x3") ? PLAN_BF16X3 : !std::strcmp(dt, "bf16_approx") ? PLAN_BF16 : -1;
        const bool shipped = !std::strcmp(kind, "shipped");
        if (dtype < 0 || (!shipped && std::strcmp(kind, "generic")) || nb < 1 || nb > PLAN_MAX_BLOCKS || (shipped && nb != 2)) {
            std::fprintf(stderr, "bad query: %s %s %d %d %d\n", dt, kind, nb, H, W);
            return 2;
        }
        const NetPlan p = plan_resnet(dtype, shipped, nb, H, W, false);
        if (!p.ok) {
            std::puts("none");
            continue;
        }
        char* o = line;
        o += std::sprintf(o, "%s lds=%zu", plan_name(p.stem), p.stem_lds.bytes);
        for (int i = 0; i < p.n_blocks; ++i) {
            const BlockPlan& b = p.block[i];
            o += std::sprintf(o, " | %s %s %d ", plan_name(b), plan_name(b.body), b.clips);
            if (b.kernel == BLOCK_X3) o += std::sprintf(o, "resblock_x3<%d,%s,G%d>", b.in.w, plan_name(b.body), b.clips);
            else if (b.kernel == BLOCK_BF16_FIXED || b.kernel == BLOCK_BF16_RUNTIME) o += std::sprintf(o, "%s<G%d>", plan_name(b), b.clips);
            else o += std::sprintf(o, "%s", plan_name(b));
            o += std::sprintf(o, " %dx%d->%dx%d lds=%zu", b.in.h, b.in.w, b.out.h, b.out.w, b.lds);
        }
        o += std::sprintf(o, " | %s | ", plan_name(p.head));
        o += put_tail(o, p);
        if (shipped && dtype != PLAN_FP32) {
            const NetPlan q = plan_resnet(dtype, shipped, nb, H, W, true);
            o += std::sprintf(o, " | pipeline: %s %s ", plan_name(q.stem), plan_name(q.head));
            o += put_tail(o, q);
        }
        std::puts(line);
    }
    return 0;
}
