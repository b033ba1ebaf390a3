// Host-only sweep of thin_route (csrc/conv_thin_route.h) over the grid of tests/test_thin_cover_cpu.py, meant to be compiled with the host
// sanitizers (build_variants.sh route_check) and run on a CPU: no device is touched, nothing is launched.  Every answer must name a kernel, a
// grid of at least one block and template arguments the launcher of conv_thin.hip has.
#include "../../gansynth_amd/csrc/conv_thin_route.h"
#include <stdio.h>

int main() {
    using namespace gs;
    const int chans[] = {1, 2, 3, 4, 8, 16, 32, 64, 96, 128, 256, 512};
    const ThinKnobs knobs[] = {thin_knobs_env(), ThinKnobs{2, 2}};
    long n = 0, bad = 0;
    for (int ks : {1, 3}) for (int mode : {MODE_S1, MODE_S2, MODE_T2}) for (int ic : chans) for (int oc : chans) for (int dtype : {GS_F32, GS_BF16})
        for (int form : {GS_THIN_PLAIN, GS_THIN_FWD_MASK, GS_THIN_BWD_PNBWD}) for (int act : {GS_ACT_NONE, GS_ACT_LRELU, GS_ACT_TANH}) for (long P : {1L, 120L, 666L, 8L * 128 * 1024})
            for (const ThinKnobs& k : knobs) {
                if (ks == 1 && mode != MODE_S1) continue;
                const ThinCall c = {mode, ks, ic, oc, dtype, P, form, act, act != GS_ACT_NONE, form == GS_THIN_FWD_MASK ? GS_ACT_LRELU : GS_ACT_NONE, dtype == GS_BF16};
                const ThinRoute r = thin_route(c, k);
                ++n;
                const bool ok = r.kernel >= GS_THIN_EXPAND && r.kernel <= GS_THIN_DIRECT && r.grid >= 1 && r.C >= 0 && r.C <= 4 && r.trips >= 0 && r.tails >= 0 && r.trips + r.tails >= 1 &&
                                (r.kernel != GS_THIN_DIRECT || (r.OCV >= 1 && r.VEC >= 1 && oc % r.OCV == 0 && ic % r.VEC == 0));
                if (!ok) { ++bad; printf("bad route: ks %d mode %d %d->%d dtype %d form %d act %d P %ld -> kernel %d grid %d\n", ks, mode, ic, oc, dtype, form, act, P, r.kernel, r.grid); }
            }
    printf(bad ? "%ld of %ld routes BAD\n" : "thin_route_check OK (%ld routes)\n", bad ? bad : n, n);
    return bad ? 1 : 0;
}
