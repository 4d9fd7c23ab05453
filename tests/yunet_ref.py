"""Test oracle for the YuNet detector (no cv2 here, so nothing is pinned to OpenCV itself):
- `run_graph`: a torch-CPU fp64 interpreter of the PARSED ONNX graph (onnx_min), independent of detector.build_plan;
- `decode_nms`: OpenCV FaceDetectorYN::postProcess + dnn::NMSBoxes (4.8+, YuNet-2023mar) restated in numpy."""
import numpy as np
import torch
import torch.nn.functional as F


def preprocess(frame_bgr: np.ndarray) -> torch.Tensor:
    """H x W x 3 uint8 BGR -> (1, 3, padH, padW) float64, zero-padded bottom / right to a multiple of 32, 0..255, no swap"""
    h, w, _ = frame_bgr.shape
    ph, pw = ((h - 1) // 32 + 1) * 32, ((w - 1) // 32 + 1) * 32
    x = torch.zeros(1, 3, ph, pw, dtype=torch.float64)
    x[0, :, :h, :w] = torch.from_numpy(frame_bgr.astype(np.float64)).permute(2, 0, 1)
    return x


def run_graph(g, x: torch.Tensor) -> dict:
    """evaluate every node of `g` in file order on the float64 input; returns the graph outputs as numpy float64"""
    env = {g.inputs[0].name: x}
    for name, t in g.initializers.items():
        env[name] = torch.from_numpy(np.array(t.array)).to(torch.float64 if t.array.dtype.kind == "f" else torch.int64)
    for n in g.nodes:
        a = [env[i] if i else None for i in n.inputs]
        op, at = n.op_type, n.attrs
        if op == "Conv":
            p = at.get("pads", (0, 0, 0, 0))
            assert p[0] == p[2] and p[1] == p[3]
            y = F.conv2d(a[0], a[1], a[2] if len(a) > 2 else None, stride=at.get("strides", (1, 1)), padding=(p[0], p[1]),
                         dilation=at.get("dilations", (1, 1)), groups=at.get("group", 1))
        elif op == "Relu":
            y = torch.relu(a[0])
        elif op == "Sigmoid":
            y = torch.sigmoid(a[0])
        elif op == "MaxPool":
            assert at.get("pads", (0, 0, 0, 0)) == (0, 0, 0, 0) and at.get("ceil_mode", 0) == 0
            y = F.max_pool2d(a[0], at["kernel_shape"], at.get("strides", at["kernel_shape"]))
        elif op == "Resize":
            assert at["mode"] == b"nearest" and at["coordinate_transformation_mode"] == b"asymmetric"
            assert at["nearest_mode"] == b"floor"
            sh, sw = (int(v) for v in a[2][2:].tolist())
            y = a[0].repeat_interleave(sh, 2).repeat_interleave(sw, 3)         # out[i] = in[floor(i / s)]
        elif op == "Add":
            y = a[0] + a[1]
        elif op == "Transpose":
            y = a[0].permute(*at["perm"])
        elif op == "Reshape":
            y = a[0].reshape([int(v) for v in a[1].tolist()])
        else:
            raise NotImplementedError(op)
        env[n.outputs[0]] = y
    return {o.name: env[o.name].numpy() for o in g.outputs}


def rect_overlap(a, b) -> np.float32:
    """cv::rectOverlap of two Rect2i: 1.f - (float)jaccardDistance, the distance in double"""
    aa, ab = int(a[2]) * int(a[3]), int(b[2]) * int(b[3])
    if aa + ab <= 0:
        return np.float32(1.0)
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    iw, ih = min(a[0] + a[2], b[0] + b[2]) - x1, min(a[1] + a[3], b[1] + b[3]) - y1
    inter = float(iw * ih) if iw > 0 and ih > 0 else 0.0
    return np.float32(1.0) - np.float32(1.0 - inter / ((aa + ab) - inter))


def decode(outs: dict, w: int, h: int, conf: float) -> np.ndarray:
    """FaceDetectorYN::postProcess up to NMS: the candidate rows (float32, N x 15) in anchor order, levels 8, 16, 32"""
    pw, ph = ((w - 1) // 32 + 1) * 32, ((h - 1) // 32 + 1) * 32
    conf = np.float32(conf)
    rows = []
    for s in (8, 16, 32):
        cols, nr = pw // s, ph // s
        cls = outs["cls_%d" % s].reshape(-1).astype(np.float32)
        obj = outs["obj_%d" % s].reshape(-1).astype(np.float32)
        bb = outs["bbox_%d" % s].reshape(-1, 4).astype(np.float32)
        kp = outs["kps_%d" % s].reshape(-1, 10).astype(np.float32)
        assert cls.size == cols * nr
        score = np.sqrt(np.clip(cls, 0, 1) * np.clip(obj, 0, 1)).astype(np.float32)
        f32 = np.float32
        for idx in np.nonzero(~(score < conf))[0]:
            r, c = divmod(int(idx), cols)
            fs, fc, fr = f32(s), f32(c), f32(r)
            cx, cy = (fc + bb[idx, 0]) * fs, (fr + bb[idx, 1]) * fs
            bw, bh = np.exp(bb[idx, 2]) * fs, np.exp(bb[idx, 3]) * fs
            row = [cx - bw / f32(2), cy - bh / f32(2), bw, bh]
            for n in range(5):
                row += [(kp[idx, 2 * n] + fc) * fs, (kp[idx, 2 * n + 1] + fr) * fs]
            rows.append(np.array(row + [score[idx]], np.float32))
    return np.array(rows, np.float32).reshape(-1, 15)


def nms(faces: np.ndarray, conf: float, nms_thr: float, top_k: int) -> np.ndarray:
    """the NMS step of FaceDetectorYN (dnn::NMSBoxes with eta 1): only for two or more candidates"""
    if faces.shape[0] <= 1:
        return faces
    boxes = faces[:, :4].astype(np.int64)                         # Rect2i(int(x), int(y), int(w), int(h)): truncation
    scores = faces[:, 14]
    cand = [i for i in range(len(faces)) if scores[i] > np.float32(conf)]
    cand.sort(key=lambda i: -scores[i])                           # stable: equal scores keep anchor order
    if top_k > 0:
        cand = cand[:top_k]
    keep = []
    for i in cand:
        if keep:
            k = boxes[keep]
            b = boxes[i]
            aa, ab = b[2] * b[3], k[:, 2] * k[:, 3]
            iw = np.minimum(b[0] + b[2], k[:, 0] + k[:, 2]) - np.maximum(b[0], k[:, 0])
            ih = np.minimum(b[1] + b[3], k[:, 1] + k[:, 3]) - np.maximum(b[1], k[:, 1])
            inter = np.where((iw > 0) & (ih > 0), iw.astype(np.float64) * ih, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                dist = (1.0 - inter / ((aa + ab) - inter)).astype(np.float32)
            ov = np.where(aa + ab <= 0, np.float32(1), np.float32(1) - dist)
            if not np.all(ov <= np.float32(nms_thr)):
                continue
        keep.append(i)
    return faces[keep].reshape(-1, 15)


def decode_nms(outs: dict, w: int, h: int, conf: float, nms_thr: float, top_k: int) -> np.ndarray:
    return nms(decode(outs, w, h, conf), conf, nms_thr, top_k)
