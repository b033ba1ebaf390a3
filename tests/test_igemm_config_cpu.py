"""CPU: the implicit-GEMM conv dispatch as a function that can be asked (gs_conv_igemm_config: host arithmetic, no launch; without a GPU the
library sizes grids for the MI355X's 256 CUs, so these answers are the device's).

tests/golden/igemm_configs.json pins, row for row, what the last branch-tree dispatch (8772697) launched for every layer shape of a sweep and
what its two `*_is_fused` entry points answered (tests/golden/record_igemm_configs.py).  A retuned threshold or a new configuration shows up
here as the exact rows that changed hands; re-record the table with the change."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "igemm_configs.json")
KNOBS = ("GS_NO_SMALL_TILES", "GS_NO_RB128", "GS_SPEC")
S1, S2, T2 = 0, 1, 2
NORM_BWD, NORM_BWD2 = 2, 3


def _config(lib, mode, n, hb, wb, ic, oc, dtype, want):
    out = (ctypes.c_int * 10)()
    rc = lib.gs_conv_igemm_config(mode, n, hb, wb, ic, oc, dtype, want, out)
    assert rc == 0, (rc, lib.gs_last_error())
    return list(out)


def _default_knobs():
    return not any(k in os.environ for k in KNOBS)


def _table():
    """The recorded table as rows: (mode, dtype, n, hb, wb, ic, oc, want, config) and (entry, mode, dtype, n, hb, wb, ic, oc, answer).
    The file holds one string per (mode, dtype, n); in it a letter per (shape, want) names the configuration ('.': the ABI has no such call),
    resp. a digit per shape gives the `*_is_fused` answer."""
    t = json.load(open(GOLDEN))
    assert t["config_fields"] == ["A", "B", "TW", "TG", "RESIDENT", "D", "NORM", "RB", "SPEC"] and t["shape_fields"] == ["hb", "wb", "ic", "oc"]
    config = dict(zip(t["config_letters"], t["config"]))
    outer = [(m, d, n) for m in t["mode"] for d in t["dtype"] for n in t["n"]]
    inner = [(s, w) for s in t["shape"] for w in t["want"]]
    assert len(t["choice"]) == len(outer) and all(len(line) == len(inner) for line in t["choice"])
    configs = [(m, d, n, *s, w, config[c]) for (m, d, n), line in zip(outer, t["choice"]) for (s, w), c in zip(inner, line) if c != "."]
    fused = []
    for entry, key in enumerate(("bwd_data_pnbwd_is_fused", "fwd_pnbwdbwd_is_fused")):
        lines = iter(t[key])
        for m, d, n in outer:
            if m in t["is_fused_modes"][entry]:
                line = next(lines)
                assert len(line) == len(t["shape"])
                fused += [(entry, m, d, n, *s, int(c)) for s, c in zip(t["shape"], line)]
        assert next(lines, None) is None
    return configs, fused


def test_chooser_reproduces_the_recorded_table():
    from gansynth_amd import _lib
    assert _default_knobs(), "the table pins the default knobs"
    lib = _lib.load()
    configs, _ = _table()
    assert len(configs) == 7480
    changed = []
    for mode, dtype, n, hb, wb, ic, oc, want, cfg in configs:
        got = _config(lib, mode, n, hb, wb, ic, oc, dtype, want)
        if got != cfg + [1]:   # (the recorded configuration, and it is compiled)
            changed.append(((mode, dtype, n, hb, wb, ic, oc, want), cfg, got))
    assert not changed, f"{len(changed)} rows changed hands, first: {changed[:5]}"


def test_is_fused_answers_are_the_recorded_ones_and_the_choosers():
    from gansynth_amd import _lib
    assert _default_knobs(), "the table pins the default knobs"
    lib = _lib.load()
    _, fused = _table()
    assert len(fused) == 2720
    entries = (lib.gs_conv_bwd_data_pnbwd_is_fused, lib.gs_conv_fwd_pnbwdbwd_is_fused)
    seen = set()
    for entry, mode, dtype, n, hb, wb, ic, oc, answer in fused:
        assert mode in ((S1, S2), (S1, T2))[entry]
        transposed = mode != S1
        ci, co = (oc, ic) if entry == 0 else (ic, oc)   # a data gradient contracts the layer's OUTPUT channels
        got = entries[entry](_lib.GsConv(n, hb, wb, ci, co, 3, 2 if transposed else 1, 1 if transposed else 0, dtype))
        want = (NORM_BWD, NORM_BWD2)[entry]
        assert got == answer, (entry, mode, dtype, n, hb, wb, ic, oc)
        assert bool(got) == (_config(lib, mode, n, hb, wb, ic, oc, dtype, want)[6] == want), (entry, mode, dtype, n, hb, wb, ic, oc)
        seen.add((entry, mode, answer))
    assert len(seen) == 8   # both answers occur for each entry point and mode


def _uncompiled():
    """Every shape of the wide sweep whose chosen configuration is NOT in the table of instantiations (run as a child: the knobs are read once)."""
    from gansynth_amd import _lib
    lib = _lib.load()
    out, rows = (ctypes.c_int * 10)(), 0
    missing = []
    chans = range(32, 513, 32)
    for mode in (S1, S2, T2):
        for dtype in (_lib.GS_F32, _lib.GS_BF16):
            for ic in chans:   # (igemm_supported: 64-byte channel chunks in, 32-channel tiles out -- every multiple of 32 passes in both dtypes)
                for oc in chans:
                    for wb in (8, 16, 32, 64, 128, 256, 512, 1024):
                        for hb in (max(1, wb // 8), wb):
                            for n in (1, 2, 4, 8, 16, 32, 64):
                                for want in range(4):
                                    rc = lib.gs_conv_igemm_config(mode, n, hb, wb, ic, oc, dtype, want, out)
                                    rows += 1
                                    if rc != 0 or out[9] != 1 or out[6] not in (0, want):
                                        missing.append([mode, dtype, n, hb, wb, ic, oc, want, rc] + list(out))
    return rows, missing


def test_every_chosen_configuration_is_compiled():
    """Totality: whatever the chooser answers, under each measurement knob set and unset, the dispatcher has an instantiation to launch."""
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    base["PYTHONPATH"] = ROOT + os.pathsep + base.get("PYTHONPATH", "")
    for knobs in ({}, {"GS_NO_SMALL_TILES": "1"}, {"GS_NO_RB128": "1"}, {"GS_SPEC": "0"}, {"GS_SPEC": "1"},
                  {"GS_NO_SMALL_TILES": "1", "GS_NO_RB128": "1", "GS_SPEC": "0"}):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env={**base, **knobs}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        rows, missing = json.loads(r.stdout.strip().splitlines()[-1])
        assert rows == 3 * 2 * 16 * 16 * 8 * 2 * 7 * 4
        assert not missing, (knobs, len(missing), missing[:5])


def test_query_refuses_what_the_implicit_gemm_does_not_take():
    from gansynth_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 10)()
    assert lib.gs_conv_igemm_config(S1, 8, 16, 128, 2, 32, _lib.GS_BF16, 0, out) == -3   # the colour block's 2 channels: not this path
    assert lib.gs_conv_igemm_config(3, 8, 16, 128, 32, 32, _lib.GS_BF16, 0, out) == -1
    assert lib.gs_conv_igemm_config(S1, 8, 16, 128, 32, 32, _lib.GS_BF16, 4, out) == -1
    assert lib.gs_conv_igemm_config(S1, 8, 16, 128, 32, 32, _lib.GS_BF16, 0, None) == -1


if __name__ == "__main__":
    print(json.dumps(_uncompiled()))
