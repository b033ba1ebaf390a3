"""GPU: the resident note bank on the device (DESIGN.md "Resident notes") -- gs_bank_gather bit for bit against tests/bank_ref.py on both
of its paths with guarded outputs, row offsets past 2^31 elements, bank_input_fn against nsynth_input_fn batch by batch, and a trainer
fed by the bank against one fed the host pipeline's batches.

Every comparison is exact: an int16 sample times 2^-15 has one fp32 value, and a label is 0 or 1."""
import ctypes

import numpy as np
import pytest
import torch

from gansynth_amd import bank, dataset
from oracle import torch_ref as R
from tests import bank_ref as BR

pytestmark = pytest.mark.gpu
ROWS = 40
GUARD = 8          # floats on either side of an output: 32 bytes, so the guarded view keeps the allocation's 16-byte alignment
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    return kernels.get()


_BANKS = {}


def small_bank(length):
    """(pcm int16 [ROWS, length], classes int32 [ROWS]) on the host, made once per length: random samples, both ends of the int16 range
    in the first and the last row, classes over 0..60 with a -1 and a 0."""
    if length not in _BANKS:
        rng = np.random.default_rng(length)
        pcm = rng.integers(-32768, 32768, size=(ROWS, length)).astype(np.int16)
        pcm[0, 0], pcm[-1, -1], pcm[5, length // 2], pcm[ROWS // 2, 0] = -32768, 32767, 32767, -32768
        classes = rng.integers(0, 61, size=ROWS).astype(np.int32)
        classes[3], classes[0], classes[-1] = -1, 0, 60
        _BANKS[length] = (pcm, classes)
    return _BANKS[length]


def an_order(batch, first):
    """first + batch entries, random rows; from 8 on the batch holds the first row twice, the last row and row 3 (class -1), a batch of
    one is the last row."""
    rng = np.random.default_rng(batch + 100 * first)
    order = rng.integers(0, ROWS, size=first + batch).astype(np.int32)
    if batch >= 8:
        order[first + np.asarray([0, 2, 5, 7])] = [0, ROWS - 1, 3, 0]
    else:
        order[first] = ROWS - 1
    return order


def guarded(shape, lead=GUARD):
    n = int(np.prod(shape))
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[lead:lead + n].view(*shape)


def intact(buf, n, lead=GUARD):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all())


def run(K, pcm_dev, classes_dev, order, first, batch, n_classes, want_waves=True, lead=GUARD):
    """gs_bank_gather into guarded outputs (the wrapper allocates its own: see the test of it below) -> (waves or None, labels) on the host."""
    rows, length = pcm_dev.shape
    order_dev = torch.from_numpy(order).cuda()
    wbuf, waves = guarded((batch, length), lead) if want_waves else (None, None)
    lbuf, labels = guarded((batch, n_classes))
    code = K.lib.gs_bank_gather(pcm_dev.data_ptr(), rows, length, pcm_dev.stride(0), classes_dev.data_ptr(), order_dev.data_ptr(), len(order),
                                first, batch, n_classes, None if waves is None else waves.data_ptr(), labels.data_ptr(),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, K.lib.gs_last_error()
    torch.cuda.synchronize()
    assert intact(lbuf, batch * n_classes), "labels: a guard was written"
    if want_waves:
        assert intact(wbuf, batch * length, lead), "waves: a guard was written"
    return (None if waves is None else waves.cpu().numpy()), labels.cpu().numpy()


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("n_classes", [61, 1])
@pytest.mark.parametrize("batch", [1, 8, 64])
@pytest.mark.parametrize("length", [64000, 1003, 8, 1])
def test_gather_is_exact(K, length, batch, n_classes):
    pcm, classes = small_bank(length)
    pcm_dev, classes_dev = torch.from_numpy(pcm).cuda(), torch.from_numpy(classes).cuda()
    for first in (0, 5):
        order = an_order(batch, first)
        want_w, want_l = BR.gather(pcm, classes, order, first, batch, n_classes)
        got_w, got_l = run(K, pcm_dev, classes_dev, order, first, batch, n_classes)
        assert same(got_w, want_w) and same(got_l, want_l), (length, batch, n_classes, first)
        none_w, only_l = run(K, pcm_dev, classes_dev, order, first, batch, n_classes, want_waves=False)
        assert none_w is None and same(only_l, want_l)
    if batch >= 8:
        assert want_w.min() == -1.0 and want_w.max() == np.float32(32767.0 / 32768.0)          # both ends of the range were drawn
        if n_classes == 61:
            assert (want_l.sum(axis=1) == 0).any() and want_l.sum() == batch - (order[5:] == 3).sum()   # row 3: class -1, an all-zero label
    # the wrapper: its own outputs, the same values
    w, lab = K.bank_gather(pcm_dev, classes_dev, torch.from_numpy(order).cuda(), 5, batch, n_classes)
    assert w.dtype == torch.float32 and w.shape == (batch, length) and lab.shape == (batch, n_classes)
    assert torch.equal(w.cpu(), torch.from_numpy(want_w)) and torch.equal(lab.cpu(), torch.from_numpy(want_l))
    w, lab = K.bank_gather(pcm_dev, classes_dev, torch.from_numpy(order).cuda(), 5, batch, n_classes, want_waves=False)
    assert w is None and torch.equal(lab.cpu(), torch.from_numpy(want_l))


@pytest.mark.parametrize("batch", [1, 8])
def test_gather_takes_the_scalar_path_for_unaligned_geometry(K, batch):
    """length 64000 is the vector path's geometry; a bank that starts one sample into its allocation, an output that starts one float
    into its own, and rows 64001 apart each send the same call down the scalar path, with the same result."""
    length = 64000
    pcm, classes = small_bank(length)
    classes_dev = torch.from_numpy(classes).cuda()
    order = an_order(batch, 2)
    want_w, want_l = BR.gather(pcm, classes, order, 2, batch, 61)
    flat = torch.zeros((ROWS * length + 1,), dtype=torch.int16, device="cuda")
    shifted = flat[1:].view(ROWS, length)
    shifted.copy_(torch.from_numpy(pcm))
    assert shifted.data_ptr() % 16 == 2
    got_w, got_l = run(K, shifted, classes_dev, order, 2, batch, 61)
    assert same(got_w, want_w) and same(got_l, want_l)
    w, lab = K.bank_gather(shifted, classes_dev, torch.from_numpy(order).cuda(), 2, batch, 61)
    assert torch.equal(w.cpu(), torch.from_numpy(want_w)) and torch.equal(lab.cpu(), torch.from_numpy(want_l))
    aligned = torch.from_numpy(pcm).cuda()
    got_w, got_l = run(K, aligned, classes_dev, order, 2, batch, 61, lead=GUARD + 1)            # waves 4 bytes off a 16-byte boundary
    assert same(got_w, want_w) and same(got_l, want_l)
    wide = torch.zeros((ROWS, length + 1), dtype=torch.int16, device="cuda")
    wide[:, :length].copy_(aligned)
    got_w, got_l = run(K, wide[:, :length], classes_dev, order, 2, batch, 61)                     # row_stride 64001
    assert same(got_w, want_w) and same(got_l, want_l)
    padded = torch.zeros((ROWS, length + 8), dtype=torch.int16, device="cuda")
    padded[:, :length].copy_(aligned)
    got_w, got_l = run(K, padded[:, :length], classes_dev, order, 2, batch, 61)                   # row_stride 64008: the vector path, strided
    assert same(got_w, want_w) and same(got_l, want_l)


def test_gather_reads_nothing_for_a_row_outside_the_bank(K):
    for length in (64000, 1003):
        pcm, classes = small_bank(length)
        pcm_dev, classes_dev = torch.from_numpy(pcm).cuda(), torch.from_numpy(classes).cuda()
        order = np.asarray([7, -1, ROWS, 0, 2 ** 31 - 1, -2 ** 31, ROWS - 1, 3], dtype=np.int32)
        want_w, want_l = BR.gather(pcm, classes, order, 0, 8, 61)
        assert not want_w[[1, 2, 4, 5]].any() and not want_l[[1, 2, 4, 5, 7]].any() and want_l.sum() == 3
        got_w, got_l = run(K, pcm_dev, classes_dev, order, 0, 8, 61)
        assert same(got_w, want_w) and same(got_l, want_l)
        # a class at or past n_classes: an all-zero label as well
        got_w, got_l = run(K, pcm_dev, classes_dev, order, 0, 8, 1)
        assert same(got_w, want_w) and same(got_l, BR.gather(pcm, classes, order, 0, 8, 1)[1])


def test_gather_offsets_past_2_to_the_31(K):
    """Row 33,554 of 64,000 samples holds element 2^31 (and byte 2^32) of the bank, row 33,603 lies wholly past it.  The 4.0 GiB
    allocation is NOT initialised: only the three rows the order names are written, so an offset that wrapped at 32 bits would come back
    with another row or with whatever the allocator left there."""
    rows, length = 33604, 64000
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"{free >> 30} GiB free: the 4.0 GiB bank and its copies need 8")
    assert 33554 * length < 2 ** 31 < 33555 * length < 33603 * length and 33554 * length * 2 < 2 ** 32 < 33555 * length * 2
    big = torch.empty((rows, length), dtype=torch.int16, device="cuda")
    rng = np.random.default_rng(31)
    picked = [0, 33554, 33603]
    data = rng.integers(-32768, 32768, size=(3, length)).astype(np.int16)
    data[:, 0], data[:, -1] = [11, 12, 13], [-32768, 32767, -1]
    for j, r in enumerate(picked):
        big[r].copy_(torch.from_numpy(data[j]))
    classes = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
    classes[torch.tensor(picked, device="cuda")] = torch.tensor([60, 0, 33], dtype=torch.int32, device="cuda")
    order = np.asarray([33603, 0, 33554, 33554], dtype=np.int32)
    want_w = data[[2, 0, 1, 1]].astype(np.float32) * np.float32(2.0 ** -15)
    want_l = np.zeros((4, 61), dtype=np.float32)
    want_l[[0, 1, 2, 3], [33, 60, 0, 0]] = 1.0
    got_w, got_l = run(K, big, classes, order, 0, 4, 61)
    assert same(got_w, want_w) and same(got_l, want_l)
    got_w, got_l = run(K, big, classes, order, 1, 3, 61, lead=GUARD + 1)                          # the scalar path's offsets too
    assert same(got_w, want_w[1:]) and same(got_l, want_l[1:])
    del big
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ the feed
FEED_PITCHES = [24, 30, 40, 41, 84, 85, 23, 60, 30, 41, 50, 61, 40, 33, 34, 35, 36, 37, 38, 39, 70, 71, 72, 73]
FEED_SOURCES = [0, 0, 1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def notes24(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("notes24")
    files, notes = BR.write_notes(tmp, 24, 64000, FEED_PITCHES, FEED_SOURCES, seed=11, split=10)
    whole, filtered = str(tmp / "whole.bank"), str(tmp / "filtered.bank")
    bank.pack(files, whole)
    bank.pack(files, filtered, pitches=range(24, 85), sources=[0])
    return files, bank.NoteBank.open(whole), bank.NoteBank.open(filtered)


def drain(fn, limit=100):
    out = []
    for _ in range(limit):
        try:
            out.append(fn())
        except StopIteration:
            return out
    raise AssertionError("the feed did not end")


@pytest.mark.parametrize("packed", ["whole", "filtered"])
@pytest.mark.parametrize("case", [dict(shuffle=True, seed=3, pitches=range(24, 85), sources=[0]),
                                  dict(shuffle=True, seed=1, buffer_size=6, pitches=range(24, 85), sources=[0]),
                                  dict(shuffle=False, pitches=[30, 40, 41, 33, 70], sources=[0]),
                                  dict(shuffle=True, seed=2, pitches=range(24, 90), sources=None)], ids=["paper", "buffered", "five pitches", "every source"])
def test_feed_yields_the_host_pipeline_batches(K, notes24, packed, case):
    files, whole, filtered = notes24
    if packed == "filtered" and case["sources"] is None:
        with pytest.raises(ValueError, match="removed when"):
            bank.bank_input_fn(filtered, batch_size=4, num_epochs=2, device="cuda", **case)
        return
    kw = dict(batch_size=4, num_epochs=2, device="cuda", **case)
    host = dataset.nsynth_input_fn(files, **kw)
    feed = bank.bank_input_fn(whole if packed == "whole" else filtered, **kw)
    assert feed.finite is True and feed.finite == host.finite
    want, got = drain(host), drain(feed)
    assert len(got) == len(want) >= 2                                                  # StopIteration at the same call
    for i, ((w0, l0), (w1, l1)) in enumerate(zip(want, got)):
        assert w1.is_cuda and w1.dtype == torch.float32 and l1.dtype == torch.float32 and w1.shape == (4, 64000)
        assert torch.equal(w0, w1) and torch.equal(l0, l1), f"batch {i}"
    usable = sum(1 for p, s in zip(FEED_PITCHES, FEED_SOURCES) if p in set(case["pitches"]) and (case["sources"] is None or s == 0))
    assert len(got) == 2 * usable // 4 and (2 * usable) % 4 != 0 and usable % 4 != 0   # a batch straddles the epochs; the remainder is dropped once
    for fn in (host, feed):
        with pytest.raises(StopIteration):
            fn()
    # next_labels: the labels of the batch a full call would have returned, and exactly one batch consumed
    mixed = bank.bank_input_fn(whole if packed == "whole" else filtered, **kw)
    with K.account() as calls:
        for i in range(len(want)):
            if i % 2 == 1:
                assert torch.equal(mixed.next_labels(), want[i][1]), f"labels of batch {i}"
            else:
                w, lab = mixed()
                assert torch.equal(w, want[i][0]) and torch.equal(lab, want[i][1]), f"batch {i} after next_labels"
        with pytest.raises(StopIteration):
            mixed.next_labels()
    assert [c[0] for c in calls] == ["bank_gather"] * len(want)                        # one launch per call, nothing else
    for i, (_, meta, read, written) in enumerate(calls):
        n_classes = want[0][1].shape[1]
        assert meta["want_waves"] == (i % 2 == 0)
        assert read == 4 * 8 + (4 * 64000 * 2 if i % 2 == 0 else 0) and written == 4 * n_classes * 4 + (4 * 64000 * 4 if i % 2 == 0 else 0)
    assert bank.bank_input_fn(whole if packed == "whole" else filtered, **dict(kw, num_epochs=None)).finite is False


def test_bank_uploads_once_in_chunks(notes24, monkeypatch):
    _, whole, _ = notes24
    fresh = bank.NoteBank.open(whole.path)
    monkeypatch.setattr(bank, "UPLOAD_CHUNK_BYTES", 5 * 64000 * 2 + 6)                 # a staging buffer that holds no whole number of rows
    dev = fresh.to("cuda")
    assert dev.dtype == torch.int16 and dev.shape == (24, 64000) and dev.is_cuda
    assert torch.equal(dev.cpu(), torch.from_numpy(np.array(fresh.pcm)))
    assert fresh.to("cuda") is dev and fresh.to(torch.device("cuda", torch.cuda.current_device())) is dev


# --------------------------------------------------------------------------------------------------------------- the trainer
SPECTRAL = dict(waveform_length=1024, sample_rate=16000, spectrogram_shape=[16, 128], overlap=0.75)
STEPS = 3


@pytest.fixture(scope="module")
def notes1024(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("notes1024")
    files, _ = BR.write_notes(tmp, 24, 1024, FEED_PITCHES, FEED_SOURCES, seed=12, split=10)
    path = str(tmp / "short.bank")
    bank.pack(files, path, length=1024, pitches=range(24, 85), sources=[0])
    return files, bank.NoteBank.open(path)


def small_gan(real_input_fn, graphs):
    """The reduced PGGAN of tests/test_ema_gpu.py (2x16 -> 16x128, 32..64 channels), fully grown, batch 4, fed 1024-sample waveforms."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pg = PGGAN(growing_level=1.0, min_resolution=[2, 16], max_resolution=[16, 128], min_channels=32, max_channels=64)
    latents = [R.synthetic_batch(4, rank=i, image_shape=(2, 16, 128))[0] for i in range(2 * STEPS)]
    calls = [0]

    def fake_input_fn():
        calls[0] += 1
        return latents[calls[0] - 1].cuda()

    hyper = dict(R.DEFAULT_HYPER, generator_learning_rate=5e-3, discriminator_learning_rate=5e-3)
    return GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, Dict(SPECTRAL), Dict(hyper), use_graphs=graphs)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_trainer_on_the_bank_follows_the_host_pipeline_bit_for_bit(K, notes1024, graphs):
    from gansynth_amd import variables
    files, short = notes1024
    kw = dict(batch_size=4, num_epochs=2, shuffle=True, pitches=range(24, 85), sources=[0], device="cuda", seed=4)   # 9 batches, 6 used
    host = dataset.nsynth_input_fn(files, **kw)          # (decodes to 64000 samples: the notes' 1024 and zeros)
    served = []

    def reference_batches():
        wav, lab = host()
        assert not wav[:, 1024:].any()
        served.append(lab)
        return wav[:, :1024].contiguous(), lab

    runs = []
    for feed in (reference_batches, bank.bank_input_fn(short, **kw)):
        model = small_gan(feed, graphs)
        variables.set_default_store(model.store)
        with K.account() as calls:
            losses = [tuple(t.detach().clone() for t in model.train_step()) for _ in range(STEPS)]
            model.synchronize()
        runs.append((model, losses, [c for c in calls if c[0] == "bank_gather"]))
    (a, losses_a, draws_a), (b, losses_b, draws_b) = runs
    assert len(served) == 2 * STEPS and draws_a == []
    # two draws per iteration: the discriminator run's whole batch, then the generator run's labels alone
    assert [d[1]["want_waves"] for d in draws_b] == [True, False] * STEPS
    for i, ((d0, g0), (d1, g1)) in enumerate(zip(losses_a, losses_b)):
        assert torch.isfinite(d0).all() and torch.isfinite(g0).all()
        assert torch.equal(d0, d1) and torch.equal(g0, g1), f"losses of step {i}"
    assert not torch.equal(losses_a[0][0], losses_a[1][0])
    for pa, pb in ((a.g_params, b.g_params), (a.d_params, b.d_params)):
        assert torch.equal(pa.flat, pb.flat) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v) and pa.t == pb.t
    assert a.global_step == b.global_step == STEPS
    assert len(drain(host)) == 9 - 2 * STEPS             # (the producer thread ends with its input)
