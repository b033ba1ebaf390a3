"""Resident notes: NSynth packed once into one file, uploaded once, every batch drawn on the device (DESIGN.md "Resident notes").

`pack(filenames, out_path)` reads the records `dataset.nsynth_input_fn` reads (the reference's `*.tfrecord` files or an
`examples.json`), decodes each note as `dataset.decode_wav` does and keeps its int16 samples.  `NoteBank.open(path)` memory-maps the
file, `.to(device)` uploads the samples once, and `bank_input_fn(bank, ...)` is `nsynth_input_fn` over the same files without the host
work: the same batches in the same order (both feeds take each epoch's order from `dataset.epoch_order`), one `gs_bank_gather` launch
per call, no thread, no queue, no pinned copy.

File layout (little endian): magic `GSNBANK1`, uint32 length of a JSON header, the header -- `rows`, `length`, `total_records` and the
pack filter `pitch_lo`, `pitch_hi`, `sources` (null: unfiltered) --, zeros to a 4096-byte boundary, then `int16 pcm[rows][length]`,
`int32 pitch[rows]`, `int32 source[rows]`, `int32 record[rows]`: the position of each row in the unfiltered record list, ascending.
"""
import json
import struct

import numpy as np
import torch

from . import dataset

MAGIC = b"GSNBANK1"
ALIGN = 4096
UPLOAD_CHUNK_BYTES = 256 << 20   # .to(device): the pinned staging buffer is at most this large
_FIELDS = ("rows", "length", "total_records", "pitch_lo", "pitch_hi", "sources")


def _data_offset(header_bytes):
    return -(-(len(MAGIC) + 4 + header_bytes) // ALIGN) * ALIGN


def pack(filenames, out_path, length=dataset.WAVEFORM_LENGTH, pitches=None, sources=None):
    """Packs the notes of `filenames` into `out_path` and returns the header.  `pitches` / `sources` drop rows at pack time
    (min(pitches) <= pitch <= max(pitches), source in sources) to keep the file small; a feed may then only ask for what was kept.
    The samples are written note by note: the set is never held in memory."""
    filenames = [filenames] if isinstance(filenames, str) else list(filenames)
    if not filenames:
        raise ValueError("bank.pack: no input files")
    length = int(length)
    if length <= 0:
        raise ValueError(f"bank.pack: length must be positive (got {length})")
    lo, hi = (None, None) if not pitches else (int(min(pitches)), int(max(pitches)))
    src_ok = None if not sources else sorted(set(int(s) for s in sources))
    records = [r for fn in filenames for r in dataset._records(fn)]   # (path, pitch, source): small; the samples are what is large
    kept = [k for k, (_, pitch, source) in enumerate(records)
            if (lo is None or lo <= pitch <= hi) and (src_ok is None or source in src_ok)]
    header = dict(rows=len(kept), length=length, total_records=len(records), pitch_lo=lo, pitch_hi=hi, sources=src_ok)
    text = json.dumps(header, sort_keys=True).encode()
    row = np.zeros(length, dtype="<i2")
    with open(out_path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", len(text)) + text)
        f.write(b"\0" * (_data_offset(len(text)) - f.tell()))
        for k in kept:
            pcm = dataset.decode_wav_pcm(records[k][0], length)
            row[:len(pcm)] = pcm
            row[len(pcm):] = 0
            f.write(row.tobytes())
        f.write(np.asarray([records[k][1] for k in kept], dtype="<i4").tobytes())
        f.write(np.asarray([records[k][2] for k in kept], dtype="<i4").tobytes())
        f.write(np.asarray(kept, dtype="<i4").tobytes())
    return header


class NoteBank(object):
    """A packed file, memory-mapped: `.pcm` int16 [rows, length], `.pitch`, `.source`, `.record` int32 [rows], `.header`."""

    def __init__(self, path, header, pcm, pitch, source, record):
        self.path, self.header = path, header
        self.rows, self.length, self.total_records = header["rows"], header["length"], header["total_records"]
        self.pcm, self.pitch, self.source, self.record = pcm, pitch, source, record
        self._resident = {}

    @classmethod
    def open(cls, path):
        """ValueError naming the field when the file is not a bank or is not as long as its header says."""
        with open(path, "rb") as f:
            head = f.read(len(MAGIC) + 4)
            if head[:len(MAGIC)] != MAGIC:
                raise ValueError(f"{path}: bad magic {head[:len(MAGIC)]!r} (a note bank starts with {MAGIC!r})")
            if len(head) < len(MAGIC) + 4:
                raise ValueError(f"{path}: truncated before the header length")
            (n,) = struct.unpack("<I", head[len(MAGIC):])
            text = f.read(n)
            f.seek(0, 2)
            size = f.tell()
        if len(text) < n:
            raise ValueError(f"{path}: header length {n} runs past the end of the file ({size} bytes)")
        try:
            header = json.loads(text.decode())
        except (UnicodeDecodeError, ValueError) as e:
            raise ValueError(f"{path}: header is not JSON ({e})")
        if not isinstance(header, dict):
            raise ValueError(f"{path}: header is not a JSON object")
        for name in _FIELDS:
            if name not in header:
                raise ValueError(f"{path}: header lacks '{name}'")
        for name in ("rows", "length", "total_records"):
            v = header[name]
            if not isinstance(v, int) or isinstance(v, bool) or v < (1 if name == "length" else 0):
                raise ValueError(f"{path}: header field '{name}' = {v!r} is not a valid count")
        rows, length = header["rows"], header["length"]
        if rows > header["total_records"]:
            raise ValueError(f"{path}: header field 'rows' = {rows} exceeds 'total_records' = {header['total_records']}")
        if rows >= 1 << 31:
            raise ValueError(f"{path}: header field 'rows' = {rows} does not fit the int32 row orders")
        if (header["pitch_lo"] is None) != (header["pitch_hi"] is None):
            raise ValueError(f"{path}: header fields 'pitch_lo' and 'pitch_hi' must both be set or both be null")
        if header["sources"] is not None and not isinstance(header["sources"], list):
            raise ValueError(f"{path}: header field 'sources' is neither null nor a list")
        off = _data_offset(n)
        want = off + rows * length * 2 + 3 * rows * 4
        if size != want:
            raise ValueError(f"{path}: file size {size} is not the {want} bytes its header claims (rows {rows}, length {length})")
        if rows == 0:
            empty = np.zeros((0,), dtype="<i4")
            return cls(path, header, np.zeros((0, length), dtype="<i2"), empty, empty, empty)
        pcm = np.memmap(path, dtype="<i2", mode="r", offset=off, shape=(rows, length))
        tail = np.memmap(path, dtype="<i4", mode="r", offset=off + rows * length * 2, shape=(3, rows))
        pitch, source, record = (np.array(tail[i]) for i in range(3))
        if record[0] < 0 or record[-1] >= header["total_records"] or (rows > 1 and not (np.diff(record) > 0).all()):
            raise ValueError(f"{path}: 'record' is not an ascending list of positions in [0, total_records = {header['total_records']})")
        return cls(path, header, pcm, pitch, source, record)

    def to(self, device):
        """The samples as an int16 device tensor [rows, length], uploaded once per device through a pinned staging buffer."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device in self._resident:
            return self._resident[device]
        out = torch.empty((self.rows, self.length), dtype=torch.int16, device=device)
        total = self.rows * self.length
        if total:
            flat_dev, flat_host = out.view(-1), self.pcm.reshape(-1)
            step = min(total, UPLOAD_CHUNK_BYTES // 2)
            stage = torch.empty((step,), dtype=torch.int16, pin_memory=device.type == "cuda")
            stage_np = stage.numpy()
            for at in range(0, total, step):
                n = min(step, total - at)
                stage_np[:n] = flat_host[at:at + n]
                flat_dev[at:at + n].copy_(stage[:n], non_blocking=True)
                if device.type == "cuda":
                    torch.cuda.current_stream(device).synchronize()   # (one staging buffer: it is refilled next)
        self._resident[device] = out
        return out


class BankFeed(object):
    """`bank_input_fn`'s callable: () -> (waveforms [B, length] fp32, labels [B, len(pitches)] fp32) on the device."""

    def __init__(self, bank, batch_size, num_epochs, shuffle, buffer_size, pitches, sources, device, seed):
        if not pitches:
            raise ValueError("bank_input_fn: `pitches` is required (the label table, dataset.py:15)")
        if int(batch_size) <= 0:
            raise ValueError(f"bank_input_fn: batch_size must be positive (got {batch_size})")
        self.bank, self.batch_size, self.num_epochs, self.shuffle = bank, int(batch_size), num_epochs, bool(shuffle)
        self.buffer_size, self.seed, self.device = buffer_size, seed, device
        table = {int(p): i for i, p in enumerate(sorted(pitches))}
        src_ok = None if not sources else set(int(s) for s in sources)
        h = bank.header
        if h["pitch_lo"] is not None:
            gone = sorted(p for p in table if not h["pitch_lo"] <= p <= h["pitch_hi"])
            if gone:
                raise ValueError(f"bank_input_fn: pitches {gone} were removed when {bank.path} was packed "
                                 f"(it keeps {h['pitch_lo']}..{h['pitch_hi']})")
        if h["sources"] is not None:
            gone = "every source" if src_ok is None else sorted(src_ok - set(h["sources"]))
            if gone:
                raise ValueError(f"bank_input_fn: sources {gone} were removed when {bank.path} was packed (it keeps {h['sources']})")
        self.n_classes = len(table)
        # the label index of every row, -1 for a row the filter drops (dataset.nsynth_input_fn: pitch in the table, source in sources)
        self.class_of_row = np.asarray([table.get(int(p), -1) for p in bank.pitch], dtype=np.int32)
        if src_ok is not None and bank.rows:
            self.class_of_row[~np.isin(bank.source, sorted(src_ok))] = -1
        self.row_of_record = np.full(bank.total_records, -1, dtype=np.int64)
        self.row_of_record[bank.record] = np.arange(bank.rows)
        if num_epochs is None and not (self.class_of_row >= 0).any():
            raise ValueError("bank_input_fn: no note passes the filter, and num_epochs=None would never end")
        self.finite = num_epochs is not None   # (models.GANSynth.train: data-parallel ranks vote before each step when the input can run dry)
        self._chunks = self._order_chunks()
        self._order, self._first = None, 0     # the uploaded row order and the next batch's position in it
        self._pcm = self._classes = None

    def _order_chunks(self):
        """One int32 array of rows per epoch, in the order nsynth_input_fn visits them: the rows an earlier epoch's last partial batch
        left over, then this epoch's, cut to whole batches.  What is cut off is carried on; at the very end it is dropped."""
        rng = np.random.default_rng(self.seed)
        carry = np.zeros((0,), dtype=np.int32)
        epoch = 0
        while self.num_epochs is None or epoch < self.num_epochs:
            rows = self.row_of_record[dataset.epoch_order(self.bank.total_records, rng, self.shuffle, self.buffer_size)]
            rows = rows[rows >= 0]
            rows = rows[self.class_of_row[rows] >= 0].astype(np.int32)
            chunk = np.concatenate([carry, rows])
            whole = len(chunk) // self.batch_size * self.batch_size
            carry = chunk[whole:]
            epoch += 1
            if whole:
                yield chunk[:whole]
            if self.bank.total_records == 0:
                break

    def row_batches(self):
        """The rows of every batch this feed's parameters draw, from the start, on the host (a fresh iterator: the feed does not move)."""
        for chunk in self._order_chunks():
            for at in range(0, len(chunk), self.batch_size):
                yield chunk[at:at + self.batch_size]

    def _advance(self):
        if self._order is None or self._first >= self._order.numel():
            chunk = next(self._chunks, None)
            if chunk is None:
                self._chunks = iter(())
                raise StopIteration
            if self._pcm is None:
                device = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
                self._pcm = self.bank.to(device)
                self._classes = torch.from_numpy(self.class_of_row).to(device)
            self._order, self._first = torch.from_numpy(chunk).to(self._pcm.device), 0   # a whole epoch at a time
        first = self._first
        self._first += self.batch_size
        return first

    def _draw(self, want_waves):
        from . import kernels
        first = self._advance()
        return kernels.get().bank_gather(self._pcm, self._classes, self._order, first, self.batch_size, self.n_classes, want_waves=want_waves)

    def __call__(self):
        return self._draw(True)

    def next_labels(self):
        """Advances one batch and returns only its labels (the generator run's draw: no waveform is read or written)."""
        return self._draw(False)[1]


def bank_input_fn(bank, batch_size, num_epochs, shuffle, buffer_size=None, pitches=None, sources=None, device=None, seed=0):
    """`dataset.nsynth_input_fn` over the files `bank` was packed from, served from the device: the same batches in the same order for
    the same arguments.  `bank`: a NoteBank or the path of a packed file.  ValueError if the filter asks for notes the pack removed."""
    if not isinstance(bank, NoteBank):
        bank = NoteBank.open(bank)
    return BankFeed(bank, batch_size, num_epochs, shuffle, buffer_size, pitches, sources, device, seed)
