"""Pitch-classifier weights without TensorFlow: the reference's frozen GraphDef (gan_synth_main.py:111-122) and .safetensors files.

GraphDef is read straight off the protobuf wire (dataset.py's reader): GraphDef{1: NodeDef} -> NodeDef{1: name, 2: op, 5: attr map}
-> attr["value"] = AttrValue{8: TensorProto} -> TensorProto{1: dtype, 2: TensorShapeProto{2: Dim{1: size}}, 4: tensor_content,
5: float_val}.  The `Const` nodes that freeze_graph made of the `resnet/...` variables are the weights.  A frozen graph also holds
the constants of the ops under the same scopes (int32 `.../Reshape/shape` and `.../moments/mean/reduction_indices`, float scalars
such as `resnet/conv/add/y`): only the variables the network asks for are taken, every other node is passed over.  A .safetensors
file is an 8-byte little-endian header length, a JSON header {name: {dtype, shape, data_offsets}} and the raw tensor bytes.
"""
import json
import os
import struct

import numpy as np

from .dataset import _fields

_DT_FLOAT, _DT_DOUBLE = 1, 2


def _shape(buf):
    return [v for num, _, dim in _fields(buf) if num == 2 for n2, _, v in _fields(dim) if n2 == 1]


def _dtype(buf):
    for num, _, val in _fields(buf):
        if num == 1:
            return val
    return 0   # (proto3 default: DT_INVALID)


def _tensor(buf, name):
    dtype, shape, content, floats = _DT_FLOAT, [], None, []
    for num, wt, val in _fields(buf):
        if num == 1:
            dtype = val
        elif num == 2:
            shape = _shape(val)
        elif num == 4:
            content = bytes(val)
        elif num == 5:   # repeated float: packed (wire type 2) or one per field (wire type 5)
            floats.extend(np.frombuffer(bytes(val), dtype="<f4").tolist())
    if dtype != _DT_FLOAT:
        raise ValueError(f"classifier variable {name}: tensor dtype {dtype} (DT_FLOAT = 1 expected)")
    numel = int(np.prod(shape)) if shape else 1
    if content is not None:
        arr = np.frombuffer(content, dtype="<f4")
        if arr.size != numel:
            raise ValueError(f"classifier variable {name}: {arr.size} values for shape {shape}")
    elif len(floats) == numel:
        arr = np.asarray(floats, dtype=np.float32)
    elif 0 < len(floats) < numel:   # TF stores a run of equal trailing values once: the last one repeats
        arr = np.concatenate([np.asarray(floats, dtype=np.float32), np.full(numel - len(floats), floats[-1], dtype=np.float32)])
    else:
        raise ValueError(f"classifier variable {name}: {len(floats)} values for shape {shape}")
    return arr.astype(np.float32).reshape(shape)


def graphdef_constants(buf, prefix="resnet/", names=None):
    """{node name: float32 array} of the float Const nodes of a serialized GraphDef whose names start with `prefix` (constants of other
    types -- shapes, reduction indices -- are passed over).  `names`: take those nodes only; one of them that is not a float tensor is
    refused by name."""
    wanted = None if names is None else set(names)
    out = {}
    for num, _, node in _fields(memoryview(bytes(buf))):
        if num != 1:
            continue
        name, op, value = None, None, None
        for n2, _, v in _fields(node):
            if n2 == 1:
                name = bytes(v).decode()
            elif n2 == 2:
                op = bytes(v).decode()
            elif n2 == 5:   # map<string, AttrValue> entry: {1: key, 2: value}
                key, attr = None, None
                for n3, _, v3 in _fields(v):
                    if n3 == 1:
                        key = bytes(v3).decode()
                    elif n3 == 2:
                        attr = v3
                if key == "value":
                    value = attr
        if op != "Const" or name is None or not name.startswith(prefix) or value is None:
            continue
        if wanted is not None and name not in wanted:
            continue
        for n4, _, v4 in _fields(value):
            if n4 == 8 and (wanted is not None or _dtype(v4) == _DT_FLOAT):
                out[name] = _tensor(v4, name)
    return out


_ST_DTYPES = {"F32": "<f4", "F64": "<f8", "F16": "<f2", "BF16": None}


def read_safetensors(path):
    with open(path, "rb") as f:
        data = f.read()
    (hlen,) = struct.unpack("<Q", data[:8])
    header = json.loads(data[8:8 + hlen].decode())
    base = 8 + hlen
    out = {}
    for name, info in header.items():
        if name == "__metadata__":
            continue
        lo, hi = info["data_offsets"]
        raw = data[base + lo:base + hi]
        if info["dtype"] == "BF16":
            arr = (np.frombuffer(raw, dtype="<u2").astype(np.uint32) << 16).view(np.float32)
        elif info["dtype"] == "I64":   # counters (a checkpoint's global_step): kept as integers
            out[name] = np.frombuffer(raw, dtype="<i8").reshape(info["shape"]).copy()
            continue
        elif info["dtype"] in _ST_DTYPES:
            arr = np.frombuffer(raw, dtype=_ST_DTYPES[info["dtype"]])
        else:
            raise ValueError(f"{path}: variable {name} has dtype {info['dtype']}")
        out[name] = arr.astype(np.float32).reshape(info["shape"])
    return out


def write_safetensors(path, tensors):
    """{name: array} -> a .safetensors file of fp32 tensors; integer arrays (counters) are stored as I64."""
    header, blobs, off = {}, [], 0
    for name, t in tensors.items():
        integer = np.issubdtype(np.asarray(t).dtype, np.integer)
        arr = np.ascontiguousarray(np.asarray(t, dtype="<i8" if integer else "<f4"))
        header[name] = {"dtype": "I64" if integer else "F32", "shape": list(arr.shape), "data_offsets": [off, off + arr.nbytes]}
        blobs.append(arr.tobytes())
        off += arr.nbytes
    h = json.dumps(header).encode()
    h += b" " * ((8 - len(h) % 8) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)))
        f.write(h)
        for b in blobs:
            f.write(b)


def load_classifier_weights(source, names=None):
    """source: a GraphDef (.pb path or bytes) or a .safetensors path -> {name: float32 array}.  `names`: the variables the network
    needs; a missing one is refused by name (shapes are checked by ResNet.load_state_dict).  From a GraphDef only those are returned
    (the graph's op constants under the same scopes are not weights); a .safetensors file is returned whole."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        weights = graphdef_constants(source, names=names)
    else:
        path = os.fspath(source)
        if path.endswith(".safetensors"):
            weights = read_safetensors(path)
        else:
            with open(path, "rb") as f:
                weights = graphdef_constants(f.read(), names=names)
    for n in names or ():
        if n not in weights:
            raise KeyError(f"classifier weights lack the variable {n}")
    return weights
