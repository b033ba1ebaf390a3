// Host-only sweep of dense_route (csrc/dense_route.h) over the grid of tests/test_dense_cover_cpu.py, for both values of the MFMA knob, meant to be
// compiled with the host sanitizers (build_variants.sh route_check) and run on a CPU: no device is touched, nothing is launched.  Every accepted
// route must name a kernel, a grid of at least one block, template constants the launchers of dense.hip have, passes that cover the batch and,
// for the forward, slices that cover the input rows; every refusal must carry a code and a reason.
#include "../../gansynth_amd/csrc/dense_route.h"
#include <set>
#include <stdio.h>

int main() {
    using namespace gs;
    const int thresholds[][4] = {{4, 4, 0, 0}, {16, 4, 16, 0}, {32, 4, 32, 0}, {64, 32, 64, 0}, {128, 4, 128, 0}, {256, 32, 64, 256}, {1024, 4, 16, 64}, {2048, 4, 64, 256}, {4096, 16, 256, 0}};
    std::set<int> widths;
    for (const auto& t : thresholds) {
        for (int v : {t[0] - 1, t[0], t[0] + 1}) widths.insert(v);
        for (int i = 1; i < 4; ++i)
            if (t[i]) { widths.insert(t[0] - t[i]); widths.insert(t[0] + t[i]); }
    }
    widths.erase(0);
    long n = 0, refused = 0, bad = 0;
    for (int map : {GS_DENSE_MAP_FWD, GS_DENSE_MAP_BWD_DATA, GS_DENSE_MAP_BWD_WEIGHT}) for (int b : {1, 5, 8, 13, 16, 17, 24, 30, 64, 65}) for (int in : widths) for (int out : widths)
        for (int dtype : {GS_F32, GS_BF16}) for (int no_mfma : {0, 1}) for (int cl : {0, 1}) {
            int rc = 0;
            if (cl) {   // a channels-last factorisation where the width has one
                for (int f : {8, 4, 2, 3, 5, 7, 11, 13}) if (!rc && in % f == 0 && in / f > 1) rc = f;
                if (!rc) continue;
            }
            DenseRoute r;
            const char* why = nullptr;
            const int e = dense_route(DenseCall{map, b, in, out, rc, rc ? in / rc : 0, dtype}, DenseKnobs{no_mfma}, &r, &why);
            ++n;
            bool ok;
            if (e) {
                ++refused;
                ok = (e == GS_ERR_ARG || e == GS_ERR_UNSUPPORTED) && why && r.kernel == 0 && r.grid_x == 0 && rc != 0;   // (plain rows are never refused)
            } else {
                const bool fb = r.FB == 8 || r.FB == 16 || r.FB == 24;
                ok = r.kernel >= GS_DENSE_FWD && r.kernel <= GS_DENSE_BWD_WEIGHT_FAST && r.kernel != GS_DENSE_FINALIZE && r.grid_x >= 1 && r.grid_y >= 1 && r.step >= 1 &&
                     (long)r.passes * r.step >= b && (long)(r.passes - 1) * r.step < b &&
                     (r.kernel == GS_DENSE_FWD_FAST ? fb && r.WPR == 0 : r.kernel == GS_DENSE_BWD_DATA_FAST ? fb && (r.WPR == 1 || r.WPR == 4) : r.FB == 0 && r.WPR == 0) &&
                     (map == GS_DENSE_MAP_FWD ? r.ksplit >= 1 && (long)r.ksplit * r.ipb >= in && (long)(r.ksplit - 1) * r.ipb < in && r.ws_bytes >= (size_t)r.ksplit * b * out * sizeof(float)
                                              : r.ksplit == 0 && r.ipb == 0 && r.finalize == 0 && r.ws_bytes == 0) &&
                     (!no_mfma || (r.kernel != GS_DENSE_FWD_MFMA && r.kernel != GS_DENSE_BWD_DATA_MFMA));
            }
            if (!ok) { ++bad; printf("bad route: map %d b %d %d->%d rc %d dtype %d no_mfma %d -> code %d kernel %d grid %d x %d FB %d WPR %d step %d passes %d ksplit %d ipb %d\n", map, b, in, out, rc, dtype, no_mfma, e, r.kernel, r.grid_x, r.grid_y, r.FB, r.WPR, r.step, r.passes, r.ksplit, r.ipb); }
        }
    printf(bad ? "%ld of %ld routes BAD\n" : "dense_route_check OK (%ld routes, %ld of them refusals)\n", bad ? bad : n, bad ? n : refused);
    return bad ? 1 : 0;
}
