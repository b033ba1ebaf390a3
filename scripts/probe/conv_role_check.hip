// Host-only walk over the one place conv geometry is decided (conv_api.hip: conv_role) and the queries built on it, meant to be compiled with
// the host sanitizers (build_variants.sh role_check) and run on a CPU: no device is touched, nothing is launched.  For every layer of the grid
// of tests/test_abi_cpu.py (_WORKSPACE_BYTES) and both dtypes it checks the role of each map against the layer's own labelling (the table in
// include/gansynth_hip.h, restated here from the layer's side) and prints the workspace sizes and both *_is_fused answers.
#include "../../gansynth_amd/csrc/conv_api.hip"
#include <stdio.h>

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { ++failures; printf("  FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

int main() {
    using namespace gs;
    const int grid[][8] = {{8, 16, 128, 32, 32, 3, 1, 0}, {8, 16, 128, 32, 32, 3, 2, 0}, {8, 8, 64, 64, 128, 3, 1, 0}, {8, 8, 64, 64, 128, 3, 2, 0},
                           {8, 16, 128, 2, 32, 1, 1, 0},  {8, 16, 128, 32, 2, 1, 1, 0},  {8, 2, 16, 1, 256, 3, 1, 0},  {8, 2, 16, 257, 256, 3, 1, 0},
                           {8, 8, 64, 64, 32, 3, 2, 1},   {8, 2, 16, 256, 256, 3, 2, 1}};
    for (const auto& g : grid)
        for (int dtype = GS_F32; dtype <= GS_BF16; ++dtype) {
            GsConv c;
            memset(&c, 0, sizeof(c));
            c.n = g[0]; c.h = g[1]; c.w = g[2]; c.ci = g[3]; c.co = g[4]; c.ksize = g[5]; c.stride = g[6]; c.transposed = g[7]; c.dtype = dtype; c.alpha = 1.f;
            EXPECT(check_conv(&c) == 0);
            const int s = c.stride, up = c.transposed;
            const int ho = up ? 2 * c.h : c.h / s, wo = up ? 2 * c.w : c.w / s;   // the layer's forward output
            const ConvRole f = conv_role(c, GS_CONV_FWD), d = conv_role(c, GS_CONV_BWD_DATA), q = conv_role(c, GS_CONV_BWD_WEIGHT);
            // forward: reads x, writes y
            EXPECT(f.mode == (up ? MODE_T2 : s == 2 ? MODE_S2 : MODE_S1) && f.variant == 0 && f.ICk == c.ci && f.OCk == c.co);
            EXPECT(f.Hi == c.h && f.Wi == c.w && f.Ho == ho && f.Wo == wo && f.Hb == (up ? c.h : ho) && f.Wb == (up ? c.w : wo));
            // data gradient: reads gy (y's shape), writes gx (x's shape); the strided maps change sides
            EXPECT(d.mode == (up ? MODE_S2 : s == 2 ? MODE_T2 : MODE_S1) && d.variant == (s == 1 ? 1 : 2) && d.ICk == c.co && d.OCk == c.ci);
            EXPECT(d.Hi == ho && d.Wi == wo && d.Ho == c.h && d.Wo == c.w && d.Hb == (up ? c.h : ho) && d.Wb == (up ? c.w : wo));
            // weight gradient: the conv from the big side to the small one; a transposed layer's with the sides swapped
            EXPECT(q.mode == (s == 2 ? MODE_S2 : MODE_S1) && q.swapped == up && q.ICk == (up ? c.co : c.ci) && q.OCk == (up ? c.ci : c.co));
            EXPECT(q.Hi == (up ? ho : c.h) && q.Wi == (up ? wo : c.w) && q.Hb == (up ? c.h : ho) && q.Wb == (up ? c.w : wo));
            printf("n %d %dx%d %d->%d k%d s%d %s %s: ws fwd %zu bwd_data %zu bwd_weight %zu, bwd_data_pnbwd fused %d, fwd_pnbwdbwd fused %d\n", c.n, c.h, c.w, c.ci, c.co,
                   c.ksize, c.stride, up ? "transposed" : "conv", dtype == GS_F32 ? "f32" : "bf16", gs_conv_workspace_bytes(&c, GS_CONV_FWD),
                   gs_conv_workspace_bytes(&c, GS_CONV_BWD_DATA), gs_conv_workspace_bytes(&c, GS_CONV_BWD_WEIGHT), gs_conv_bwd_data_pnbwd_is_fused(&c),
                   gs_conv_fwd_pnbwdbwd_is_fused(&c));
        }
    GsConv bad;   // refused layers: the queries answer 0 and touch nothing
    memset(&bad, 0, sizeof(bad));
    EXPECT(gs_conv_workspace_bytes(&bad, GS_CONV_BWD_WEIGHT) == 0 && gs_conv_workspace_bytes(nullptr, GS_CONV_FWD) == 0);
    EXPECT(gs_conv_bwd_data_pnbwd_is_fused(&bad) == 0 && gs_conv_fwd_pnbwdbwd_is_fused(nullptr) == 0);
    printf(failures ? "%d checks FAILED\n" : "conv_role_check OK\n", failures);
    return failures ? 1 : 0;
}
