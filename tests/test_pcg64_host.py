"""CPU: tests/pcg64_ref.py - numpy's PCG64 stream, Lemire's bounded draw and the stratified-bootstrap rows in plain integers - equals
numpy itself: the rows ``np.array_equal`` to the ``rng.choice`` loop, the final ``bit_generator.state`` equal (``uinteger`` only where
``has_uint32`` is set: numpy leaves a stale value there otherwise), and tests/golden/eval_draw.json - what numpy 2.2.6 drew - reproduced
by the numpy that runs here, so that a changed stream shows as a fixture mismatch."""
import hashlib

import numpy as np
import pytest

from conftest import load_json
import pcg64_ref as R

# (a, b, B, seed) -> the words a fresh default_rng(seed) consumes beyond B (a' + b'): the rejections, checked when the issue was written
CASES = {(300, 218, 7, 42): 0, (1, 7, 5, 43): 0, (16384, 5000, 3, 44): 0, (9973, 6007, 24, 3): 2, (11000, 5000, 24, 7): 3, (9973, 6007, 24, 0): 0}
STARTS = (0, 1)                       # 1: after a choice(arange(100), 40, replace=False), which leaves a buffered half-word


def start_rng(seed, buffered):
    rng = np.random.default_rng(seed)
    if buffered:
        rng.choice(np.arange(100), 40, replace=False)
    return rng


def pools(a, b):
    return np.arange(a), a + np.arange(b)


def numpy_rows(rng, a, b, B):
    pos, neg = pools(a, b)
    return np.concatenate([np.concatenate([rng.choice(pos, a, True), rng.choice(neg, b, True)]) for _ in range(B)])


def same_state(got, want):
    return (got["bit_generator"] == want["bit_generator"] and got["state"] == want["state"] and got["has_uint32"] == want["has_uint32"]
            and (not want["has_uint32"] or got["uinteger"] == want["uinteger"]))


def accepted_words(a, b, B):
    return B * ((a if a > 1 else 0) + (b if b > 1 else 0))


_statement = {}


def statement(case, buffered):
    """(start state, rows, consumed, final state) of a case by the statement, made once per session (tests/test_hip_draw.py shares it)"""
    key = (case, buffered)
    if key not in _statement:
        a, b, B, seed = case
        start = start_rng(seed, buffered).bit_generator.state
        _statement[key] = (start,) + R.draw_rows(start, a, a, b, b, B, *pools(a, b))
    return _statement[key]


def test_a_buffered_half_is_left_by_the_second_start():
    assert [start_rng(42, s).bit_generator.state["has_uint32"] for s in STARTS] == [0, 1]


@pytest.mark.parametrize("buffered", STARTS)
@pytest.mark.parametrize("case", list(CASES))
def test_rows_and_final_state_equal_numpy(case, buffered):
    a, b, B, seed = case
    rng = start_rng(seed, buffered)
    start, got, consumed, final = statement(case, buffered)
    want = numpy_rows(rng, a, b, B)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert same_state(final, rng.bit_generator.state)
    excess = consumed - accepted_words(a, b, B)
    print("case %s buffered %d: %d words, %d rejected" % (case, buffered, consumed, excess))
    assert excess >= 0
    if not buffered:
        assert excess == CASES[case]                      # the rejection path ran where the table says it does
    assert rng.random() == np.random.Generator(restored(final)).random()


def restored(sd):
    bg = np.random.PCG64()
    bg.state = sd
    return bg


def test_scalar_and_vectorised_statements_agree():
    for case in ((300, 218, 7, 42), (1, 7, 5, 43), (9973, 6007, 2, 3)):
        a, b, B, seed = case
        for buffered in STARTS:
            start = start_rng(seed, buffered).bit_generator.state
            v, s = R.draw_rows(start, a, a, b, b, B), R.draw_rows_scalar(start, a, a, b, b, B)
            assert np.array_equal(v[0], s[0]) and v[1:] == s[1:]
    start = start_rng(9, 1).bit_generator.state
    v, s = R.draw_rows(start, 2 ** 31 + 1, 257, 3 * 2 ** 30, 130, 2), R.draw_rows_scalar(start, 2 ** 31 + 1, 257, 3 * 2 ** 30, 130, 2)
    assert np.array_equal(v[0], s[0]) and v[1:] == s[1:] and v[1] > 1.5 * 774      # about half of the words are rejected


@pytest.mark.parametrize("buffered", STARTS)
@pytest.mark.parametrize("m", [2 ** 31 + 1, 3 * 2 ** 30, 2 ** 32 - 1, 2])
def test_value_mode_equals_integers(m, buffered):
    rng = start_rng(11, buffered)
    start = rng.bit_generator.state
    want = rng.integers(0, m, size=1500)
    got, consumed, final = R.draw_rows(start, m, 1500, 1, 0, 1)
    assert np.array_equal(got, want) and same_state(final, rng.bit_generator.state)
    thr = 2 ** 32 % m
    print("m %d: %d words for 1500 values, 2^32 mod m = %d" % (m, consumed, thr))
    assert consumed >= 1500 and (thr != 0 or consumed == 1500)
    if m in (2 ** 31 + 1, 3 * 2 ** 30):
        assert consumed >= 1.25 * 1500                    # 25 to 50 % of the words are rejected at these bounds


def test_a_bound_of_one_takes_no_word_and_2_pow_32_is_refused():
    start = start_rng(5, 1).bit_generator.state
    got, consumed, final = R.draw_rows(start, 1, 9, 1, 4, 3, [7], [8])
    assert got.tolist() == ([7] * 9 + [8] * 4) * 3 and consumed == 0 and final == R.pack(*R.unpack(start))
    for bad in (0, 2 ** 32, -1):
        with pytest.raises(ValueError):
            R.draw_rows(start, bad, 1, 2, 1, 1)
    with pytest.raises(ValueError):
        R.draw_rows(start, 5, 4, 2, 1, 1, items_a=[1, 2, 3])


@pytest.mark.parametrize("k", [0, 1, 2, 3, 1000, 2 ** 31 + 12345, 2 ** 64 + 17, 2 ** 127 + 5])
def test_advance_equals_numpys(k):
    bg = np.random.PCG64(77)
    s0 = bg.state
    bg.advance(k)
    assert R.advance(s0["state"]["state"], s0["state"]["inc"], k) == bg.state["state"]["state"]
    if k <= 1000:
        s = s0["state"]["state"]
        for _ in range(k):
            s = R.step(s, s0["state"]["inc"])
        assert s == bg.state["state"]["state"]


def test_outputs_equal_numpys_raw_stream():
    bg = np.random.PCG64(123)
    sd = bg.state
    raw = bg.random_raw(50)
    w = R.words(sd, 100)
    assert np.array_equal(w[0::2] | (w[1::2] << np.uint64(32)), raw)


def test_the_recorded_fixture_is_reproduced():
    doc = load_json("eval_draw.json")
    assert len(doc["cases"]) == 2 * len(CASES) and doc["numpy"] == "2.2.6"
    for c in doc["cases"]:
        case = (c["a"], c["b"], c["B"], c["seed"])
        rng = start_rng(c["seed"], c["buffered"])
        sd = rng.bit_generator.state
        assert hex(sd["state"]["state"]) == c["start"]["state"] and hex(sd["state"]["inc"]) == c["start"]["inc"], "numpy %s seeds another state" % np.__version__
        assert (sd["has_uint32"], sd["uinteger"] if sd["has_uint32"] else 0) == (c["start"]["has_uint32"], c["start"]["uinteger"] if c["start"]["has_uint32"] else 0)
        start, got, consumed, final = statement(case, c["buffered"])
        flat = got.astype("<i4")
        assert flat[:8].tolist() == c["first8"] and flat[-8:].tolist() == c["last8"]
        assert hashlib.sha256(flat.tobytes()).hexdigest() == c["sha256"], "numpy %s draws another stream than %s" % (np.__version__, doc["numpy"])
        assert consumed == c["consumed"]
        assert hex(final["state"]["state"]) == c["final"]["state"] and final["has_uint32"] == c["final"]["has_uint32"]
        assert not final["has_uint32"] or final["uinteger"] == c["final"]["uinteger"]
