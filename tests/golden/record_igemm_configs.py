"""Records tests/golden/igemm_configs.json: which implicit-GEMM tile configuration the conv dispatch of a GIVEN commit picks for every layer
shape of a sweep, and what its two `*_is_fused` entry points answer -- the table tests/test_igemm_config_cpu.py holds the chooser to.

The commit to pin has no way to tell its choice without launching, so it is recorded from a patched build that never launches:

    git worktree add /tmp/pin <commit> && cd /tmp/pin
    patch -p1 < <this repo>/tests/golden/igemm_record.patch      # launch_igemm notes its template arguments and returns
    bash gansynth_amd/csrc/build.sh
    python <this repo>/tests/golden/record_igemm_configs.py --tree /tmp/pin

No GPU is needed: on a host without one the dispatch sizes its grids for 256 CUs, the MI355X's count.  The pointers handed to the entry points
are never dereferenced (weights "prepared", no kernel runs).  The committed table was recorded at 8772697, the last commit whose dispatch was a
tree of branches.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gansynth_amd import _lib  # noqa: E402  (prototypes only: the library loaded is the patched tree's)
from tests.igemm_cover import api_call, layer_args  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
S1, S2, T2 = 0, 1, 2
PLAIN, NORM_FWD, NORM_BWD, NORM_BWD2 = 0, 1, 2, 3
CFG_FIELDS = ["A", "B", "TW", "TG", "RESIDENT", "D", "NORM", "RB", "SPEC"]
MODES, DTYPES, NS, WANTS = (S1, S2, T2), (_lib.GS_F32, _lib.GS_BF16), (1, 4, 8, 16), (PLAIN, NORM_FWD, NORM_BWD, NORM_BWD2)
LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"   # one per distinct configuration; '.': the ABI has no call for that row


def shapes():
    """(hb, wb, ic, oc): every pyramid level with the networks' channel counts as same-width, halving and doubling pairs, then a few off-pyramid."""
    chans = [256, 128, 64, 32]
    pairs = [(c, c) for c in chans] + [(2 * c, c) for c in chans[1:]] + [(c, 2 * c) for c in chans[1:]]
    out = [(2 << k, 16 << k, ic, oc) for k in range(7) for ic, oc in pairs]
    out += [(hb, wb, ic, oc) for hb, wb in [(16, 16), (6, 24), (64, 24)] for ic, oc in [(32, 96), (96, 96), (32, 128), (64, 96), (96, 32)]]
    return out


def layer_is_fused(entry, mode, n, hb, wb, ic, oc, dtype):
    """Kernel-role shape -> the layer (GsConv) the `*_is_fused` entry point is asked about for it."""
    transposed = mode != S1
    ci, co = (oc, ic) if entry == 0 else (ic, oc)   # a data gradient contracts the layer's OUTPUT channels
    return _lib.GsConv(n, hb, wb, ci, co, 3, 2 if transposed else 1, 1 if transposed else 0, dtype)


FUSED_MODES = {0: (S1, S2), 1: (S1, T2)}   # the igemm mode behind each entry point, plain / transposed layer


def drive(lib, mode, dtype, n, hb, wb, ic, oc, want):
    """Calls the entry point that reaches the dispatch with this kernel-role shape and epilogue (tests/igemm_cover.py: api_call says which map of
    which layer that is and layer_args turns the shape into the layer's); False where the ABI has none."""
    call = api_call(mode, want)
    if call is None:
        return False   # (no data gradient runs as the transposed kernel with a norm behind it)
    P = ctypes.c_void_p(0x10000)   # never dereferenced
    act, eps = _lib.ACT_LRELU, 1e-8
    c = _lib.GsConv(*layer_args(call, n, hb, wb, ic, oc), 3, call.stride, call.transposed, dtype, 1, 1.0, P, 1 << 30)
    if want == PLAIN and call.data_grad:
        lib.gs_conv_bwd_data(c, P, P, None, 0, P, None)
    elif want == PLAIN:
        lib.gs_conv_fwd(c, P, P, None, _lib.ACT_NONE, P, None, 0.0, None)
    elif want == NORM_FWD:
        lib.gs_conv_fwd(c, P, P, None, act, P, P, eps, None)
    elif want == NORM_BWD:
        lib.gs_conv_bwd_data_pnbwd(c, P, P, P, None, act, eps, P, None)
    else:
        lib.gs_conv_fwd_pnbwdbwd(c, P, P, P, P, act, eps, P, P, None)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="checkout with igemm_record.patch applied and built")
    ap.add_argument("--out", default=os.path.join(HERE, "igemm_configs.json"))
    a = ap.parse_args()
    for k in ("GS_NO_SMALL_TILES", "GS_NO_RB128", "GS_SPEC"):
        assert k not in os.environ, f"{k} is set: the table pins the default knobs"
    lib = ctypes.CDLL(os.path.join(a.tree, "gansynth_amd", "libgansynth_hip.so"))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    rec = (ctypes.c_int * 18)()
    distinct, choice, fused = [], [], [[], []]
    for mode in MODES:   # one line of the table per (mode, dtype, n): a letter per (shape, want)
        for dtype in DTYPES:
            for n in NS:
                line, answers = "", ["", ""]
                for hb, wb, ic, oc in shapes():
                    for want in WANTS:
                        lib.gs_igemm_record_get(rec)   # (clears it)
                        if not drive(lib, mode, dtype, n, hb, wb, ic, oc, want):
                            line += "."
                            continue
                        lib.gs_igemm_record_get(rec)
                        r = list(rec)
                        assert r[0] == 1, f"the dispatch was not reached: {(mode, dtype, n, hb, wb, ic, oc, want)}: {lib.gs_last_error()}"
                        assert r[1:9] == [mode, dtype, n, hb, wb, ic, oc, want], (r, (mode, dtype, n, hb, wb, ic, oc, want))
                        if r[9:] not in distinct:
                            distinct.append(r[9:])
                        line += LETTERS[distinct.index(r[9:])]
                    for entry, fn in enumerate((lib.gs_conv_bwd_data_pnbwd_is_fused, lib.gs_conv_fwd_pnbwdbwd_is_fused)):
                        if mode in FUSED_MODES[entry]:
                            answers[entry] += str(fn(layer_is_fused(entry, mode, n, hb, wb, ic, oc, dtype)))
                choice.append(line)
                for entry in (0, 1):
                    if mode in FUSED_MODES[entry]:
                        fused[entry].append(answers[entry])
    rows = lambda v: "[\n  " + ",\n  ".join(json.dumps(r, separators=(",", ":")) for r in v) + "]"   # noqa: E731
    with open(a.out, "w") as f:
        f.write('{"order": "one string per (mode, dtype, n), in that nesting; within it one character per (shape, want) resp. per shape",\n')
        f.write(' "mode": %s, "dtype": %s, "n": %s, "want": %s,\n' % tuple(json.dumps(list(v)) for v in (MODES, DTYPES, NS, WANTS)))
        sh = [list(x) for x in shapes()]
        levels = [sh[i:i + 10] for i in range(0, 70, 10)] + [sh[i:i + 5] for i in range(70, len(sh), 5)]   # one (hb, wb) per line
        f.write(' "shape_fields": ["hb", "wb", "ic", "oc"],\n "shape": [\n  %s],\n' % ",\n  ".join(json.dumps(v, separators=(",", ":"))[1:-1] for v in levels))
        f.write(' "config_fields": %s,\n "config_letters": "%s",\n "config": %s,\n' % (json.dumps(CFG_FIELDS), LETTERS[:len(distinct)], rows(distinct)))
        f.write(' "choice": %s,\n' % rows(choice))
        f.write(' "is_fused_modes": %s,\n' % json.dumps([list(FUSED_MODES[0]), list(FUSED_MODES[1])]))
        f.write(' "bwd_data_pnbwd_is_fused": %s,\n "fwd_pnbwdbwd_is_fused": %s}\n' % (rows(fused[0]), rows(fused[1])))
    print(f"{sum(len(x) - x.count('.') for x in choice)} configurations, {sum(len(x) for e in fused for x in e)} is_fused answers -> {a.out}")


if __name__ == "__main__":
    main()
