"""Three scripted calls for CallServer(tracker="device") / RealtimeCall(tracker="device") against the host tracker
(tests/test_hip_device_tracker.py j, k) and for the condition of that equality (tests/test_device_tracker_host.py f).

  A  96 x 131 B, G, R, ``detect_every=2``: every other tick has no detection; one face, and from tick 10 a row under ``start_conf``
  B  80 x 112 R, G, B, ``detect_size=(48, 36)``: the rows are found on the small frame and scaled back by 112 / 48 and 80 / 36; one
     face, and a row that is under ``start_min_size`` after the scale-back
  C  96 x 128 B, G, R: two faces, the second leaves after tick 17; detects on every tick
The detector is a stub that knows a call by the shape of the frame it is shown and answers with that call's next rows."""
import numpy as np

TICKS = 26
START_CONF, START_MIN_SIZE = 0.76, 20
CALLS = {"A": dict(shape=(96, 131), order="bgr", seed=21, detect_every=2, detect_size=None),
         "B": dict(shape=(80, 112), order="rgb", seed=22, detect_every=1, detect_size=(48, 36)),
         "C": dict(shape=(96, 128), order="bgr", seed=23, detect_every=1, detect_size=None)}
_STD = np.array([[0.3, 0.35], [0.7, 0.35], [0.5, 0.55], [0.35, 0.75], [0.65, 0.75]])


def _row(rng, x, y, w, h, score, jitter):
    j = rng.uniform(-jitter, jitter, 4)
    x, y, w, h = x + j[0], y + j[1], w + j[2], h + j[3]
    lm = _STD * [w, h] + [x, y] + rng.normal(0, 0.1 * jitter, (5, 2))
    return np.concatenate([[x, y, w, h], [score + rng.uniform(-0.004, 0.004)], lm.ravel()])


def scripted(name):
    """``[(frame, rows at the detector's size (n, 15) float32)]`` per tick of the call"""
    c = CALLS[name]
    rng = np.random.default_rng(c["seed"])
    out = []
    for s in range(TICKS):
        frame = rng.integers(0, 256, c["shape"] + (3,), dtype=np.uint8)
        if name == "A":
            rows = [_row(rng, 20 + 0.6 * s, 24 + 0.2 * s, 30, 34, 0.95, 0.3)]
            if s >= 10:
                rows.append(_row(rng, 80, 40, 28, 30, 0.60, 0.3))                       # under start_conf: never tracked
        elif name == "B":
            rows = [_row(rng, 8 + 0.3 * s, 9 + 0.1 * s, 13, 15, 0.94, 0.12)]            # 30 x 33 after the scale-back
            rows.append(_row(rng, 34, 20, 6, 7, 0.97, 0.05))                            # 14 x 16 after it: under start_min_size
        else:
            rows = [_row(rng, 14 + 0.5 * s, 22 + 0.1 * s, 30, 34, 0.95, 0.3)]
            if s < 18:
                rows.append(_row(rng, 72 - 0.4 * s, 40 + 0.3 * s, 28, 32, 0.93, 0.3))
        out.append((frame, np.asarray(rows, dtype=np.float32)))
    return out


def scripts():
    return {name: scripted(name) for name in CALLS}


def detect_ticks(name):
    """the call's own ticks on which it detects"""
    return [s for s in range(TICKS) if s % CALLS[name]["detect_every"] == 0]


def seen_shape(name):
    """the (H, W) of the frame the detector is shown for this call"""
    c = CALLS[name]
    return c["shape"] if c["detect_size"] is None else (c["detect_size"][1], c["detect_size"][0])
