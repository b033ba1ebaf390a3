"""CPU: the host layers of the resident note bank (DESIGN.md "Resident notes") -- the packer and the file's validation, the order
contract of bank_input_fn against nsynth_input_fn over the same files, the refusals of gs_bank_gather (no launch) and of its wrapper,
and the drivers' --pack_bank on a machine without a device."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from gansynth_amd import bank, dataset
from tests import bank_ref as BR

LENGTH = 200


# ------------------------------------------------------------------------------------------------------------- the packer
@pytest.fixture(scope="module")
def dozen(tmp_path_factory):
    """Twelve notes: mono and stereo, shorter than LENGTH, exactly LENGTH and longer; pitches inside and outside 24..84, two sources.
    Nine are listed in two tfrecord files, three in an examples.json."""
    tmp = tmp_path_factory.mktemp("dozen")
    rng = np.random.default_rng(7)
    sizes = [LENGTH, 50, 300, LENGTH, 1, 199, 201, LENGTH, 120]
    stereo = [False, False, False, True, False, True, True, False, False]
    pitches = [60, 23, 24, 84, 85, 40, 40, 61, 30]
    sources = [0, 0, 1, 0, 0, 2, 0, 0, 1]
    recs = []
    for i, (n, st, p, s) in enumerate(zip(sizes, stereo, pitches, sources)):
        pcm = rng.integers(-32768, 32768, size=(n, 2 if st else 1)).astype(np.int16)
        pcm[0, 0] = [-32768, 32767][i % 2]                      # both ends of the range
        path = str(tmp / f"n{i}.wav")
        BR.write_wav(path, pcm.reshape(-1), channels=2 if st else 1)
        recs.append((path, p, s))
    BR.write_tfrecord(str(tmp / "a.tfrecord"), recs[:5])
    BR.write_tfrecord(str(tmp / "b.tfrecord"), recs[5:])
    notes = {"zither_002": (50, 0, rng.integers(-32768, 32768, size=2 * 260), 2), "alto_001": (70, 1, rng.integers(-32768, 32768, size=90), 1),
             "mallet_003": (24, 0, rng.integers(-32768, 32768, size=LENGTH), 1)}
    index = BR.write_examples_json(tmp / "nsynth", notes)
    base = os.path.join(os.path.dirname(os.path.abspath(index)), "audio")
    recs += [(os.path.join(base, name + ".wav"), notes[name][0], notes[name][1]) for name in sorted(notes)]   # examples.json: sorted by name
    return tmp, [str(tmp / "a.tfrecord"), str(tmp / "b.tfrecord"), index], recs


def check_rows(b, recs, kept):
    assert (b.rows, b.length, b.total_records) == (len(kept), LENGTH, len(recs))
    assert b.pcm.shape == (len(kept), LENGTH) and b.pcm.dtype == np.int16
    assert b.record.tolist() == kept
    assert b.pitch.tolist() == [recs[k][1] for k in kept] and b.source.tolist() == [recs[k][2] for k in kept]
    for row, k in enumerate(kept):
        want = np.round(dataset.decode_wav(recs[k][0], LENGTH).astype(np.float64) * 32768.0)
        assert np.array_equal(b.pcm[row].astype(np.float64), want), recs[k][0]
        # ... and back: the gather's arithmetic on the packed row is decode_wav's value, bit for bit
        assert np.array_equal((b.pcm[row].astype(np.float32) * np.float32(2.0 ** -15)).view(np.int32),
                              dataset.decode_wav(recs[k][0], LENGTH).view(np.int32))


def test_pack_round_trip(dozen):
    tmp, files, recs = dozen
    out = str(tmp / "all.bank")
    header = bank.pack(files, out, length=LENGTH)
    assert header == dict(rows=12, length=LENGTH, total_records=12, pitch_lo=None, pitch_hi=None, sources=None)
    b = bank.NoteBank.open(out)
    assert b.header == header
    check_rows(b, recs, list(range(12)))
    raw = open(out, "rb").read()
    assert raw[:8] == b"GSNBANK1"
    (n,) = struct.unpack("<I", raw[8:12])
    assert json.loads(raw[12:12 + n]) == header and n + 12 <= 4096 and not any(raw[12 + n:4096])
    assert len(raw) == 4096 + 12 * LENGTH * 2 + 3 * 12 * 4
    assert np.array_equal(np.frombuffer(raw, dtype="<i2", count=12 * LENGTH, offset=4096).reshape(12, LENGTH), b.pcm)
    assert np.frombuffer(raw, dtype="<i4", offset=4096 + 12 * LENGTH * 2).reshape(3, 12).tolist() == \
        [b.pitch.tolist(), b.source.tolist(), b.record.tolist()]
    # one record file alone, and a single name instead of a list
    one = str(tmp / "json.bank")
    assert bank.pack(files[2], one, length=LENGTH)["rows"] == 3
    check_rows(bank.NoteBank.open(one), recs[9:], [0, 1, 2])


def test_filtered_pack_keeps_the_right_rows(dozen):
    tmp, files, recs = dozen
    out = str(tmp / "filtered.bank")
    header = bank.pack(files, out, length=LENGTH, pitches=range(24, 85), sources=[0])
    kept = [k for k, (_, p, s) in enumerate(recs) if 24 <= p <= 84 and s == 0]
    assert kept == [0, 3, 6, 7, 10, 11]
    assert header == dict(rows=6, length=LENGTH, total_records=12, pitch_lo=24, pitch_hi=84, sources=[0])
    check_rows(bank.NoteBank.open(out), recs, kept)
    by_source = str(tmp / "sources.bank")
    assert bank.pack(files, by_source, length=LENGTH, sources=[1, 2])["rows"] == 4
    check_rows(bank.NoteBank.open(by_source), recs, [2, 5, 8, 9])


def test_open_refuses_a_damaged_file(dozen):
    tmp, files, _ = dozen
    out = str(tmp / "damaged_src.bank")
    bank.pack(files, out, length=LENGTH)
    raw = open(out, "rb").read()

    def refused(data, match):
        path = str(tmp / "damaged.bank")
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError, match=match):
            bank.NoteBank.open(path)

    refused(raw[:-2], "file size")                                  # truncated
    refused(raw[:4096 + 5 * LENGTH * 2], "file size")
    refused(raw[:10], "truncated")
    refused(raw + b"\0\0\0\0", "file size")                         # too long
    refused(b"GSNBANK2" + raw[8:], "magic")
    refused(b"RIFF", "magic")
    (n,) = struct.unpack("<I", raw[8:12])
    header = json.loads(raw[12:12 + n])

    def with_header(h):
        text = json.dumps(h, sort_keys=True).encode()
        assert len(text) + 12 <= 4096
        return raw[:8] + struct.pack("<I", len(text)) + text + b"\0" * (4096 - 12 - len(text)) + raw[4096:]

    bank.NoteBank.open(out)
    refused(with_header(dict(header, rows=11)), "file size")       # a wrong size in the header
    refused(with_header(dict(header, length=LENGTH + 1)), "file size")
    refused(with_header(dict(header, length=0)), "'length'")
    refused(with_header(dict(header, rows=-1)), "'rows'")
    refused(with_header(dict(header, total_records=11)), "'rows'")
    refused(with_header({k: v for k, v in header.items() if k != "total_records"}), "'total_records'")
    refused(raw[:8] + struct.pack("<I", 1 << 30) + raw[12:], "header length")
    refused(raw[:12] + b"{" * n + raw[12 + n:], "JSON")
    swapped = bytearray(raw)
    swapped[-8:-4], swapped[-4:] = raw[-4:], raw[-8:-4]            # record[] out of order
    refused(bytes(swapped), "'record'")


# --------------------------------------------------------------------------------------------------------- the order contract
COUNT, BATCH = 13, 4   # 13 notes in batches of 4 over two epochs: a batch straddles the epoch boundary, the last two notes are dropped
NOTE_PITCHES = [24, 30, 40, 41, 84, 85, 23, 60, 30, 41, 50, 61, 40]
NOTE_SOURCES = [0, 0, 1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def thirteen(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("thirteen")
    files, notes = BR.write_notes(tmp, COUNT, 40, NOTE_PITCHES, NOTE_SOURCES, seed=3, split=6)
    whole, filtered = str(tmp / "whole.bank"), str(tmp / "filtered.bank")
    bank.pack(files, whole, length=64)
    bank.pack(files, filtered, length=64, pitches=range(24, 85), sources=[0])
    return files, notes, bank.NoteBank.open(whole), bank.NoteBank.open(filtered)


def host_sequence(files, **kw):
    """[(note numbers of the batch, label indices)] of every batch nsynth_input_fn yields; sample 0 of note i is i + 1."""
    fn = dataset.nsynth_input_fn(files, **kw)
    out = []
    while True:
        try:
            wav, lab = fn()
        except StopIteration:
            break
        assert float(lab.sum()) == lab.shape[0]
        out.append(((wav[:, 0].double() * 32768).long() - 1).tolist() + lab.argmax(dim=1).tolist())
    with pytest.raises(StopIteration):
        fn()
    return out


def bank_sequence(b, **kw):
    feed = bank.bank_input_fn(b, **kw)
    out = []
    for rows in feed.row_batches():
        assert rows.dtype == np.int32 and len(rows) == kw["batch_size"]
        assert [int(b.pcm[r, 0]) - 1 for r in rows] == b.record[rows].tolist()     # the row holds the file its record names
        out.append(b.record[rows].tolist() + feed.class_of_row[rows].tolist())
    return out, feed


FILTERS = {"paper": dict(pitches=range(24, 85), sources=[0]), "three pitches": dict(pitches=[41, 30, 40], sources=None),
           "three pitches, one source": dict(pitches=[41, 30, 40], sources=[0]), "all sources": dict(pitches=range(20, 90), sources=None)}


@pytest.mark.parametrize("packed", ["whole", "filtered"])
@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("shuffle, buffer_size", [(False, None), (True, None), (True, 5), (True, 1), (True, 100)])
def test_bank_feed_draws_what_the_host_pipeline_yields(thirteen, packed, filt, shuffle, buffer_size):
    files, notes, whole, filtered = thirteen
    kw = dict(batch_size=BATCH, num_epochs=2, shuffle=shuffle, buffer_size=buffer_size, seed=5, **FILTERS[filt])
    if packed == "filtered" and FILTERS[filt]["sources"] is None:
        with pytest.raises(ValueError, match="removed when"):   # every source (and for one filter pitches too) against a pack of source 0
            bank.bank_input_fn(filtered, **kw)
        return
    want = host_sequence(files, **kw)
    got, feed = bank_sequence(whole if packed == "whole" else filtered, **kw)
    usable = sum(1 for p, s in zip(NOTE_PITCHES, NOTE_SOURCES) if p in set(FILTERS[filt]["pitches"]) and (FILTERS[filt]["sources"] is None or s == 0))
    assert len(want) == 2 * usable // BATCH and usable % BATCH != 0 and len(want) >= 2      # (the cases do straddle and do drop)
    assert got == want                                                                       # same files, same order, same end
    assert feed.finite is True and feed.n_classes == len(set(FILTERS[filt]["pitches"]))
    if shuffle and buffer_size != 1 and usable > 4:
        assert got != bank_sequence(whole if packed == "whole" else filtered, **dict(kw, shuffle=False))[0]


def test_bank_feed_epochs_and_refusals(thirteen):
    files, notes, whole, filtered = thirteen
    paper = FILTERS["paper"]
    for epochs in (1, 3):
        kw = dict(batch_size=3, num_epochs=epochs, shuffle=True, seed=1, **paper)
        assert bank_sequence(whole, **kw)[0] == host_sequence(files, **kw)
    endless = bank.bank_input_fn(whole, batch_size=BATCH, num_epochs=None, shuffle=True, **paper)
    assert endless.finite is False
    it = endless.row_batches()
    assert len([next(it) for _ in range(40)]) == 40
    assert bank.bank_input_fn(whole, batch_size=50, num_epochs=2, shuffle=False, **paper).finite
    assert list(bank.bank_input_fn(whole, batch_size=50, num_epochs=2, shuffle=False, **paper).row_batches()) == []
    with pytest.raises(ValueError, match="pitches"):
        bank.bank_input_fn(filtered, batch_size=2, num_epochs=1, shuffle=False, pitches=range(23, 85), sources=[0])
    with pytest.raises(ValueError, match="sources"):
        bank.bank_input_fn(filtered, batch_size=2, num_epochs=1, shuffle=False, pitches=range(24, 85), sources=[0, 1])
    with pytest.raises(ValueError, match="pitches"):
        bank.bank_input_fn(whole, batch_size=2, num_epochs=1, shuffle=False, pitches=None)
    with pytest.raises(ValueError, match="never end"):
        bank.bank_input_fn(whole, batch_size=2, num_epochs=None, shuffle=False, pitches=[99])
    with pytest.raises(ValueError, match="batch_size"):
        bank.bank_input_fn(whole, batch_size=0, num_epochs=1, shuffle=False, pitches=[40])


def test_epoch_order_is_the_one_helper_both_feeds_call():
    import inspect
    assert "epoch_order(" in inspect.getsource(dataset.nsynth_input_fn) and "rng.shuffle" not in inspect.getsource(dataset.nsynth_input_fn)
    assert "dataset.epoch_order(" in inspect.getsource(bank.BankFeed._order_chunks)
    a, b = np.random.default_rng(3), np.random.default_rng(3)
    full = dataset.epoch_order(10, a, True)
    want = np.arange(10)
    b.shuffle(want)
    assert full.tolist() == want.tolist()
    assert dataset.epoch_order(10, a, False).tolist() == list(range(10))
    buffered = dataset.epoch_order(10, a, True, 3)
    assert sorted(buffered.tolist()) == list(range(10)) and all(v <= i + 2 for i, v in enumerate(buffered.tolist()))


# ---------------------------------------------------------------------------------------------------- ABI without a GPU
def test_bank_gather_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(pcm=P, rows=40, length=64000, row_stride=64000, class_of_row=P, order=P, n_order=100, first=92, batch=8, n_classes=61,
                waves=P, labels=P, stream=None)
    order = ["pcm", "rows", "length", "row_stride", "class_of_row", "order", "n_order", "first", "batch", "n_classes", "waves", "labels", "stream"]
    bad = [("pcm", None, b"pcm is null"), ("class_of_row", None, b"class_of_row is null"), ("order", None, b"order is null"),
           ("labels", None, b"labels is null"), ("rows", 0, b"rows"), ("rows", -4, b"rows"), ("length", 0, b"length"), ("length", -1, b"length"),
           ("batch", 0, b"batch"), ("batch", -8, b"batch"), ("n_classes", 0, b"n_classes"), ("n_classes", -1, b"n_classes"),
           ("row_stride", 63999, b"row_stride"), ("first", -1, b"first"), ("first", 93, b"first"), ("n_order", 99, b"first"),
           ("first", 1 << 40, b"first"), ("pcm", P + 1, b"pcm is not 2-byte"), ("waves", P + 2, b"waves is not 4-byte"),
           ("labels", P + 1, b"labels is not 4-byte"), ("labels", P + 2, b"labels is not 4-byte")]
    for field, value, message in bad:
        args = dict(good, **{field: value})
        assert lib.gs_bank_gather(*[args[k] for k in order]) == -1, (field, value)       # GS_ERR_ARG
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())


def test_bank_gather_wrapper_refuses_wrong_tensors():
    from gansynth_amd import kernels
    call = kernels.HipKernels.bank_gather   # (the checks come before the library is touched: no instance, no device)
    pcm, cls, order = torch.zeros((4, 16), dtype=torch.int16), torch.zeros((4,), dtype=torch.int32), torch.zeros((8,), dtype=torch.int32)
    for args, match in (((pcm.float(), cls, order), "pcm must be"), ((pcm[0], cls, order), "pcm must be"), ((pcm, cls.long(), order), "class_of_row"),
                        ((pcm, cls[:3], order), "class_of_row"), ((pcm, cls, order.float()), "order"), ((pcm, cls, order[::2]), "order"),
                        ((pcm, cls, order), "HIP device")):
        with pytest.raises(ValueError, match=match):
            call(None, *args, 0, 4, 3)


# ----------------------------------------------------------------------------------------------------------- the drivers
@pytest.mark.parametrize("driver", ["gan_synth_main", "pitch_classifier_main"])
def test_driver_packs_without_a_device(thirteen, tmp_path, monkeypatch, driver):
    import importlib
    main = importlib.import_module(driver)
    files, notes, _, _ = thirteen

    def no_device(*a, **kw):
        raise AssertionError("--pack_bank touched the device")

    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    out = str(tmp_path / "driver.bank")
    args = main.parser.parse_args(["--pack_bank", out, "--filenames", os.path.join(os.path.dirname(files[0]), "*.tfrecord")])
    assert args.bank is None and main.parser.parse_args(["--bank", "x.bank"]).bank == "x.bank" and main.parser.parse_args([]).pack_bank is None
    main.main(args)
    b = bank.NoteBank.open(out)
    kept = [k for k, (p, s) in enumerate(zip(NOTE_PITCHES, NOTE_SOURCES)) if 24 <= p <= 84 and s == 0]
    assert (b.rows, b.length, b.total_records) == (len(kept), 64000, COUNT) and b.record.tolist() == kept
    assert b.header["pitch_lo"] == 24 and b.header["pitch_hi"] == 84 and b.header["sources"] == [0]
    for row, k in enumerate(kept):
        assert np.array_equal(b.pcm[row, :40], notes[k][3]) and not b.pcm[row, 40:].any()
    with pytest.raises(SystemExit, match="matches no file"):
        main.main(main.parser.parse_args(["--pack_bank", out, "--filenames", str(tmp_path / "none*.tfrecord")]))
