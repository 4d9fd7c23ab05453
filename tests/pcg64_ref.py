"""numpy's PCG64 stream and its bounded draws, stated in plain Python integers: what csrc/af_draw.hip computes on the device.

State: ``bit_generator.state`` of a ``default_rng`` - ``state`` and ``inc`` (128 bit each), ``has_uint32`` and ``uinteger``.
    64-bit output j (j >= 1)   s_j = s_(j-1) MULT + inc (mod 2^128);  out_j = rotr64(hi64(s_j) ^ lo64(s_j), s_j >> 122)     (XSL-RR 128/64)
    32-bit words w[k]          the buffered ``uinteger`` first where ``has_uint32`` is set; then, of every output, lo32 before hi32
    a draw with bound m        2 <= m <= 2^32 - 1: take a word w, p = w m; where lo32(p) < 2^32 mod m take the next word, else the value
                               is hi32(p).  m == 1: the value is 0 and NO word is taken.  (2^32 takes another path in numpy: refused.)
    row r                      count_a draws with bound_a, then count_b draws with bound_b, rows one after another on the same stream
After the last word numpy holds the high half of the last output in ``uinteger`` (stale where ``has_uint32`` is 0).

``draw_rows`` is vectorised per segment over a word array made by the scalar ``step`` / ``output``; ``draw_rows_scalar`` is the same
thing one word at a time, and tests/test_pcg64_host.py holds both against numpy itself."""
import numpy as np

MULT = 0x2360ED051FC65DA44385DF649FCCF645
M128, M64, M32 = (1 << 128) - 1, (1 << 64) - 1, (1 << 32) - 1
MAX_BOUND = M32


def step(s: int, inc: int) -> int:
    return (s * MULT + inc) & M128


def output(s: int) -> int:
    x, r = ((s >> 64) ^ s) & M64, s >> 122
    return ((x >> r) | (x << ((64 - r) & 63))) & M64


def jump(inc: int, k: int):
    """k steps as one map s -> A s + C: -> (A, C), O(log k)"""
    a, c, A, C = MULT, inc, 1, 0
    while k:
        if k & 1:
            A, C = (A * a) & M128, (C * a + c) & M128
        a, c = (a * a) & M128, ((a + 1) * c) & M128
        k >>= 1
    return A, C


def advance(s: int, inc: int, k: int) -> int:
    """the state k outputs on (``PCG64.advance(k)``)"""
    A, C = jump(inc, k)
    return (A * s + C) & M128


def unpack(sd):
    """a ``bit_generator.state`` dict -> (state, inc, has_uint32, uinteger)"""
    if sd["bit_generator"] != "PCG64":
        raise ValueError("pcg64_ref: a PCG64 state, got %s" % sd["bit_generator"])
    return int(sd["state"]["state"]), int(sd["state"]["inc"]), int(sd["has_uint32"]), int(sd["uinteger"])


def pack(s, inc, has, uinteger):
    return {"bit_generator": "PCG64", "state": {"state": int(s), "inc": int(inc)}, "has_uint32": int(has), "uinteger": int(uinteger)}


def words(sd, n: int) -> np.ndarray:
    """the first n 32-bit words of the stream (uint64 array)"""
    s, inc, has, uinteger = unpack(sd)
    outs = []
    for _ in range((max(n - has, 0) + 1) // 2):
        s = step(s, inc)
        outs.append(output(s))
    o = np.array(outs, np.uint64)
    w = np.empty(2 * len(outs), np.uint64)
    w[0::2], w[1::2] = o & np.uint64(M32), o >> np.uint64(32)
    if has:
        w = np.concatenate([np.array([uinteger], np.uint64), w])
    return w[:n]


def state_after(sd, consumed: int):
    """the state dict after `consumed` words were taken"""
    s, inc, has, uinteger = unpack(sd)
    if consumed == 0:
        return pack(s, inc, has, uinteger)
    made = consumed - has                                  # words that came out of 64-bit outputs
    outputs = (made + 1) // 2
    if outputs:
        s = advance(s, inc, outputs)
        uinteger = output(s) >> 32
    return pack(s, inc, made & 1, uinteger)


def check_bound(m):
    if not 1 <= int(m) <= MAX_BOUND:
        raise ValueError("pcg64_ref: a bound of %d (1 to 2^32 - 1)" % m)
    return int(m)


def bounded(next_word, m: int) -> int:
    """one draw: `next_word()` yields the stream's next 32-bit word"""
    if m == 1:
        return 0
    thr = (1 << 32) % m
    while True:
        p = next_word() * m
        if (p & M32) >= thr:
            return p >> 32


def draw_rows_scalar(sd, bound_a, count_a, bound_b, count_b, rows, items_a=None, items_b=None):
    bound_a, bound_b = check_bound(bound_a), check_bound(bound_b)
    s, inc, has, uinteger = unpack(sd)
    st = {"s": s, "has": has, "u": uinteger, "n": 0}

    def next_word():
        st["n"] += 1
        if st["has"]:
            st["has"] = 0
            return st["u"]
        st["s"] = step(st["s"], inc)
        o = output(st["s"])
        st["has"], st["u"] = 1, o >> 32
        return o & M32
    out = []
    for _ in range(rows):
        for m, c, items in ((bound_a, count_a, items_a), (bound_b, count_b, items_b)):
            for _ in range(c):
                v = bounded(next_word, m)
                out.append(v if items is None else int(items[v]))
    return np.array(out, np.int64), st["n"], pack(st["s"], inc, st["has"], st["u"])


def _take(W, p, m, c):
    """c accepted draws with bound m from the words W[p:] -> (values, words taken), or None where W runs out"""
    thr, mm = np.uint64((1 << 32) % m), np.uint64(m)
    width = c + 16
    while True:
        win = W[p:p + width] * mm
        ok = (win & np.uint64(M32)) >= thr
        have = int(ok.sum())
        if have >= c:
            end = int(np.searchsorted(np.cumsum(ok), c)) + 1        # the word that gives the c-th value is the last one taken
            return (win[:end][ok[:end]] >> np.uint64(32)).astype(np.int64), end
        if p + width >= len(W):
            return None
        width *= 2


def draw_rows(sd, bound_a, count_a, bound_b, count_b, rows, items_a=None, items_b=None):
    """-> (flat int64 array in numpy's order, words consumed, final state dict); ``items_*`` None: the raw values ("value mode")"""
    bound_a, bound_b = check_bound(bound_a), check_bound(bound_b)
    segs = [(bound_a, int(count_a), None if items_a is None else np.asarray(items_a)),
            (bound_b, int(count_b), None if items_b is None else np.asarray(items_b))]
    for m, c, items in segs:
        if items is not None and len(items) != m:
            raise ValueError("pcg64_ref: a bound of %d over %d items" % (m, len(items)))
    T = rows * sum(c for m, c, _ in segs if m > 1)
    slack = 64
    while True:
        W, p, out = words(sd, T + slack), 0, []
        for _ in range(rows):
            for m, c, items in segs:
                if c == 0:
                    continue
                if m == 1:
                    vals = np.zeros(c, np.int64)
                else:
                    got = _take(W, p, m, c)
                    if got is None:
                        break
                    vals, used = got
                    p += used
                out.append(vals if items is None else items[vals].astype(np.int64))
            else:
                continue
            break
        else:
            flat = np.concatenate(out) if out else np.zeros(0, np.int64)
            return flat, p, state_after(sd, p)
        slack = 4 * slack + T
