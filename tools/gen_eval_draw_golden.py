"""Writes tests/golden/eval_draw.json: what NUMPY ITSELF draws for the cases tests/test_pcg64_host.py and tests/test_hip_draw.py hold the
PCG64 statement (tests/pcg64_ref.py) and the device draw (csrc/af_draw.hip) against.

    python tools/gen_eval_draw_golden.py

For every case (a, b, B, seed), from a fresh ``default_rng(seed)`` and again after a ``choice(np.arange(100), 40, replace=False)`` that
leaves a buffered half-word: the numpy version, the start state, the first and last 8 indices of the flat rows
``[rng.choice(pos, a, True), rng.choice(neg, b, True)] x B`` over ``pos = arange(a)``, ``neg = a + arange(b)``, the sha256 of the rows as
little-endian int32, the 32-bit words consumed (read off the final state) and the final state.  A numpy whose stream differs from the
recorded one then shows as a fixture mismatch, not as a kernel bug.  Needs numpy only; the 128-bit integers are written as hex strings."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pcg64_ref as R             # noqa: E402

CASES = [(300, 218, 7, 42), (1, 7, 5, 43), (16384, 5000, 3, 44), (9973, 6007, 24, 3), (11000, 5000, 24, 7), (9973, 6007, 24, 0)]


def hex_state(sd):
    return {"state": hex(sd["state"]["state"]), "inc": hex(sd["state"]["inc"]), "has_uint32": int(sd["has_uint32"]), "uinteger": int(sd["uinteger"])}


def start_rng(seed, buffered):
    rng = np.random.default_rng(seed)
    if buffered:
        rng.choice(np.arange(100), 40, replace=False)
    return rng


def numpy_rows(rng, a, b, B):
    pos, neg = np.arange(a), a + np.arange(b)
    rows = [np.concatenate([rng.choice(pos, a, True), rng.choice(neg, b, True)]) for _ in range(B)]
    return np.concatenate(rows).astype("<i4")


def words_between(start, final):
    """32-bit words taken between two states of one stream: the outputs between them, found by stepping, and the buffer flags"""
    s, inc, has, _ = R.unpack(start)
    target, outputs = int(final["state"]["state"]), 0
    while s != target:
        s, outputs = R.step(s, inc), outputs + 1
    return 2 * outputs + has - int(final["has_uint32"])


def main():
    cases = []
    for a, b, B, seed in CASES:
        for buffered in (0, 1):
            rng = start_rng(seed, buffered)
            start = rng.bit_generator.state
            flat = numpy_rows(rng, a, b, B)
            final = rng.bit_generator.state
            cases.append({"a": a, "b": b, "B": B, "seed": seed, "buffered": buffered, "start": hex_state(start), "final": hex_state(final),
                          "first8": flat[:8].tolist(), "last8": flat[-8:].tolist(), "sha256": hashlib.sha256(flat.tobytes()).hexdigest(),
                          "consumed": words_between(start, final)})
    doc = {"tool": "gen_eval_draw_golden", "numpy": np.__version__, "cases": cases}
    path = os.path.join(ROOT, "tests", "golden", "eval_draw.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
