"""A minimal ONNX reader: the protobuf wire format walked by hand (stdlib + numpy, no onnx / protobuf package).

It decodes what a small inference graph needs - ModelProto -> GraphProto: nodes (op_type, inputs, outputs, attributes),
initializers (dims, data type, raw_data or the typed repeated fields), graph inputs and outputs with their shapes - and
nothing else.  Field numbers are those of onnx.proto (opset-independent)."""
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

# TensorProto.DataType -> numpy
_DTYPES = {1: np.float32, 2: np.uint8, 3: np.int8, 5: np.int16, 6: np.int32, 7: np.int64, 9: np.bool_, 10: np.float16,
           11: np.float64, 12: np.uint32, 13: np.uint64}


def _varint(buf: bytes, pos: int) -> Tuple[int, int]:
    v = shift = 0
    while True:
        if pos >= len(buf):
            raise ValueError("truncated varint")
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if b < 0x80:
            return v, pos
        shift += 7


def _fields(buf: bytes):
    """yield (field number, wire type, value) of one message; value = int (varint / fixed) or bytes (length-delimited)"""
    pos, n = 0, len(buf)
    while pos < n:
        key, pos = _varint(buf, pos)
        fno, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            v = buf[pos:pos + 8]
            pos += 8
        elif wt == 2:
            ln, pos = _varint(buf, pos)
            v = buf[pos:pos + ln]
            if len(v) != ln:
                raise ValueError("truncated field %d" % fno)
            pos += ln
        elif wt == 5:
            v = buf[pos:pos + 4]
            pos += 4
        else:
            raise ValueError("unsupported wire type %d (field %d)" % (wt, fno))
        yield fno, wt, v


def _signed(v: int) -> int:
    return v - (1 << 64) if v >= 1 << 63 else v


def _ints(wt, v) -> List[int]:
    """a repeated int64 field element: packed (wire type 2) or one varint"""
    if wt == 0:
        return [_signed(v)]
    out, pos = [], 0
    while pos < len(v):
        x, pos = _varint(v, pos)
        out.append(_signed(x))
    return out


def _floats(wt, v) -> List[float]:
    if wt == 5:
        return [struct.unpack("<f", v)[0]]
    return list(struct.unpack("<%df" % (len(v) // 4), v))


@dataclass
class Tensor:
    name: str
    dims: Tuple[int, ...]
    array: np.ndarray


@dataclass
class Node:
    op_type: str
    name: str
    inputs: List[str]
    outputs: List[str]
    attrs: Dict[str, object] = field(default_factory=dict)


@dataclass
class ValueInfo:
    name: str
    elem_type: int
    shape: Tuple[object, ...]       # int or the symbolic name (str) per dimension


@dataclass
class Graph:
    nodes: List[Node]
    initializers: Dict[str, Tensor]
    inputs: List[ValueInfo]
    outputs: List[ValueInfo]
    opset: int
    name: str = ""


def _tensor(buf: bytes) -> Tensor:
    dims, dt, name, raw = [], 1, "", None
    typed: Dict[int, list] = {}
    for fno, wt, v in _fields(buf):
        if fno == 1:
            dims += _ints(wt, v)
        elif fno == 2:
            dt = v
        elif fno == 8:
            name = v.decode()
        elif fno == 9:
            raw = v
        elif fno in (4, 5, 7, 10, 11):                       # float_data, int32_data, int64_data, double_data, uint64_data
            if fno == 4:
                typed.setdefault(4, []).extend(_floats(wt, v))
            elif fno == 10:
                typed.setdefault(10, []).extend(struct.unpack("<%dd" % (len(v) // 8), v) if wt == 2 else struct.unpack("<d", v))
            else:
                typed.setdefault(fno, []).extend(_ints(wt, v))
    if dt not in _DTYPES:
        raise ValueError("tensor %r: unsupported data type %d" % (name, dt))
    npt = np.dtype(_DTYPES[dt]).newbyteorder("<")
    if raw is not None:
        arr = np.frombuffer(raw, dtype=npt).astype(_DTYPES[dt])
    else:
        vals = next(iter(typed.values()), [])
        arr = np.asarray(vals, dtype=_DTYPES[dt])
    count = int(np.prod(dims)) if dims else 1
    if arr.size != count:
        raise ValueError("tensor %r: %d values for dims %s" % (name, arr.size, dims))
    return Tensor(name, tuple(dims), arr.reshape(dims))


def _attribute(buf: bytes):
    name, val = "", None
    ints, floats = [], []
    for fno, wt, v in _fields(buf):
        if fno == 1:
            name = v.decode()
        elif fno == 2:
            val = struct.unpack("<f", v)[0]
        elif fno == 3:
            val = _signed(v)
        elif fno == 4:
            val = bytes(v)
        elif fno == 5:
            val = _tensor(v)
        elif fno == 7:
            floats += _floats(wt, v)
        elif fno == 8:
            ints += _ints(wt, v)
    if ints:
        val = tuple(ints)
    elif floats:
        val = tuple(floats)
    return name, val


def _node(buf: bytes) -> Node:
    n = Node("", "", [], [])
    for fno, wt, v in _fields(buf):
        if fno == 1:
            n.inputs.append(v.decode())
        elif fno == 2:
            n.outputs.append(v.decode())
        elif fno == 3:
            n.name = v.decode()
        elif fno == 4:
            n.op_type = v.decode()
        elif fno == 5:
            k, a = _attribute(v)
            n.attrs[k] = a
    return n


def _value_info(buf: bytes) -> ValueInfo:
    name, et, shape = "", 0, []
    for fno, wt, v in _fields(buf):
        if fno == 1:
            name = v.decode()
        elif fno == 2:                                          # TypeProto
            for f2, _, tt in _fields(v):
                if f2 != 1:                                     # tensor_type only
                    continue
                for f3, _, x in _fields(tt):
                    if f3 == 1:
                        et = x
                    elif f3 == 2:                               # TensorShapeProto
                        for f4, _, d in _fields(x):
                            if f4 != 1:
                                continue
                            dim: Optional[object] = None
                            for f5, _, dv in _fields(d):
                                dim = _signed(dv) if f5 == 1 else dv.decode()
                            shape.append(dim)
    return ValueInfo(name, et, tuple(shape))


def parse_model(data: bytes) -> Graph:
    """decode a serialized ModelProto"""
    graph_buf, opset = None, 0
    for fno, wt, v in _fields(data):
        if fno == 7:
            graph_buf = v
        elif fno == 8:
            dom, ver = "", 0
            for f2, _, x in _fields(v):
                if f2 == 1:
                    dom = x.decode()
                elif f2 == 2:
                    ver = x
            if dom in ("", "ai.onnx"):
                opset = ver
    if graph_buf is None:
        raise ValueError("not an ONNX model: no graph")
    g = Graph([], {}, [], [], opset)
    for fno, wt, v in _fields(graph_buf):
        if fno == 1:
            g.nodes.append(_node(v))
        elif fno == 2:
            g.name = v.decode()
        elif fno == 5:
            t = _tensor(v)
            g.initializers[t.name] = t
        elif fno == 11:
            g.inputs.append(_value_info(v))
        elif fno == 12:
            g.outputs.append(_value_info(v))
    return g


def load(path: str) -> Graph:
    with open(path, "rb") as f:
        return parse_model(f.read())
