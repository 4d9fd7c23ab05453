"""Compares the host-side conv decisions of two builds of libafhip.so over a grid of descriptors well outside the networks' own.

    python tools/sweep_conv_paths.py <libafhip.so of the parent> <libafhip.so under test>

For a refactor of the conv launchers: every answer of the second library must equal the first one's.  No GPU is
needed - a machine without a device counts 256 compute units.  Build the parent's library as tools/gen_conv_paths_golden.py says.

Layers: dtype x n x t x (h = w) x cin x cout x {1x1x1, 3x1x1, 1x3x3, 3x3x3 with their natural padding} x stride {1, (1,2,2), 2} x
tpool x relu, alone and with a 1x1x1 second segment of 64 or cin channels that lands on the same output positions; per call
af_conv_variant, af_conv_work_units (rc, units, workgroups, and af_last_error where it refuses) and af_conv_workspace_bytes.
(None of the device-free functions takes an out_ld or a residual, so the grid has no such axes.)
Pairs, formed from the same values: c / a (af_conv_ca_fusable, af_conv_ca_work_units; with and without the projection shortcut),
c / pool / a (af_conv_cpa_*, x_sub 0..3), b / c (af_conv_bc_fusable) and a / b / c (af_block_abc_*, also under AF_ABC_INNER32=1).
Prints the number of calls and how many gave each answer; exit status 1 if any answer differs or a path / fusion is reached by
fewer than 20 grid points.
"""
import collections
import ctypes as C
import itertools
import os
import sys

FIELDS = ("n", "t", "h", "w", "cin", "cout", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw", "to", "ho", "wo", "relu", "dtype", "tpool")
DTYPES, NS, TS, HWS = (0, 1, 2), (1, 4, 16, 64), (4, 8, 16, 32), (7, 14, 28, 56)
CHANNELS = (8, 16, 32, 64, 128, 256, 512, 1024)
KERNELS = ((1, 1, 1), (3, 1, 1), (1, 3, 3), (3, 3, 3))
STRIDES = ((1, 1, 1), (1, 2, 2), (2, 2, 2))
SPECIALISED = {4: "conv133", 8: "conv311", 9: "conv_small", 10: "conv111", 11: "conv133g", 13: "conv311g"}
MIN_REACHED = 20


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in FIELDS]


def fill(d, dtype, n, t, hw, cin, cout, kernel=(1, 1, 1), stride=(1, 1, 1), relu=1, tpool=0):
    pad = tuple(k // 2 for k in kernel)
    d.dtype, d.n, d.t, d.h, d.w, d.cin, d.cout = dtype, n, t, hw, hw, cin, cout
    d.kt, d.kh, d.kw = kernel
    d.st, d.sh, d.sw = stride
    d.pt, d.ph, d.pw = pad
    d.to, d.ho, d.wo = ((x + 2 * p - k) // s + 1 for x, p, k, s in zip((t, hw, hw), pad, kernel, stride))
    d.relu, d.tpool = relu, tpool


class Lib:
    def __init__(self, path):
        L = self.L = C.CDLL(os.path.abspath(path))
        P = C.POINTER(ConvDesc)
        L.af_last_error.restype = C.c_char_p
        L.af_conv_workspace_bytes.restype = C.c_int64
        L.af_conv_variant.argtypes = [P, P]
        L.af_conv_work_units.argtypes = [P, P, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.af_conv_workspace_bytes.argtypes = [P]
        L.af_conv_ca_fusable.argtypes = [P] * 3
        L.af_conv_ca_work_units.argtypes = [P] * 3 + [C.POINTER(C.c_int64)] + [C.POINTER(C.c_int)] * 3
        L.af_conv_cpa_fusable.argtypes = [P] * 2 + [C.c_int]
        L.af_conv_cpa_work_units.argtypes = [P] * 2 + [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.af_conv_bc_fusable.argtypes = [P] * 2
        L.af_block_abc_fusable.argtypes = [P] * 4
        L.af_block_abc_work_units.argtypes = [P] * 4 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_int64)]
        self.n64, self.i, self.j, self.k = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self.refs = [C.byref(x) for x in (self.n64, self.i, self.j, self.k)]

    def _outs(self, *which):
        for x in which:
            x.value = -7
        return which

    def layer(self, d, d2):
        L, (n64, i, _, _) = self.L, self.refs
        self._outs(self.n64, self.i)
        v = L.af_conv_variant(d, d2)
        rc = L.af_conv_work_units(d, d2, n64, i)
        work = (rc, self.n64.value, self.i.value) if rc >= 0 else (rc, L.af_last_error())
        return v, work, (L.af_conv_workspace_bytes(d) if d2 is None else None)

    def ca(self, dc, d1, da):
        n64, i, j, k = self.refs
        self._outs(self.n64, self.i, self.j, self.k)
        yes = self.L.af_conv_ca_fusable(dc, d1, da)
        return yes, self.L.af_conv_ca_work_units(dc, d1, da, n64, i, j, k), self.n64.value, self.i.value, self.j.value, self.k.value

    def cpa(self, dc, da, x_sub):
        n64, i, _, _ = self.refs
        self._outs(self.n64, self.i)
        yes = self.L.af_conv_cpa_fusable(dc, da, x_sub)
        return yes, self.L.af_conv_cpa_work_units(dc, da, x_sub, n64, i), self.n64.value, self.i.value

    def bc(self, db, dc):
        return (self.L.af_conv_bc_fusable(db, dc),)

    def abc(self, da, db, dc, d1):
        n64, i, j, _ = self.refs
        self._outs(self.n64, self.i, self.j)
        yes = self.L.af_block_abc_fusable(da, db, dc, d1)
        return yes, self.L.af_block_abc_work_units(da, db, dc, d1, i, j, n64), self.i.value, self.j.value, self.n64.value


class Sweep:
    def __init__(self, parent, branch):
        self.libs = (Lib(parent), Lib(branch))
        self.calls = collections.Counter()
        self.answers = collections.defaultdict(collections.Counter)
        self.different = []

    def ask(self, what, describe, *args):
        a, b = (getattr(lib, what)(*args) for lib in self.libs)
        self.calls[what] += 1
        if a != b:
            if len(self.different) < 20:
                self.different.append((what, describe(), a, b))
            self.answers[what]["DIFFERENT"] += 1
        return a

    def layers(self):
        d, d2 = ConvDesc(), ConvDesc()
        rd, rd2 = C.byref(d), C.byref(d2)
        show = lambda: ([getattr(d, f) for f in FIELDS], [getattr(d2, f) for f in FIELDS])
        variants, refusals = self.answers["af_conv_variant"], self.answers["af_conv_work_units refused"]
        for dtype, n, t, hw, cin, cout, kernel, stride in itertools.product(DTYPES, NS, TS, HWS, CHANNELS, CHANNELS, KERNELS, STRIDES):
            fill(d, dtype, n, t, hw, cin, cout, kernel, stride)
            if d.to <= 0 or d.ho <= 0 or d.wo <= 0:
                continue
            for tpool, relu in itertools.product((0, 1, 2), (0, 1)):
                d.tpool, d.relu = tpool, relu
                v, work, ws = self.ask("layer", show, rd, None)
                variants[v] += 1
                refusals[work[1] if work[0] < 0 else "answered"] += 1
                self.answers["af_conv_workspace_bytes"]["split K" if ws else "0"] += 1
                for cin2 in {64, cin}:      # the second segment reads the layer's input, or a 64-channel one, at the layer's stride
                    fill(d2, dtype, n, t, hw, cin2, cout, (1, 1, 1), stride, relu)
                    v, work, _ = self.ask("layer", show, rd, rd2)
                    self.answers["af_conv_variant, two segments"][v] += 1

    def pairs(self):
        da, db, dc, d1 = ConvDesc(), ConvDesc(), ConvDesc(), ConvDesc()
        ra, rb, rc, r1 = (C.byref(x) for x in (da, db, dc, d1))
        show = lambda: [[getattr(x, f) for f in FIELDS] for x in (da, db, dc, d1)]
        for dtype, n, t, hw in itertools.product(DTYPES, NS, TS, HWS):
            for cin, mid, cout, relu in itertools.product(CHANNELS, CHANNELS, CHANNELS, (0, 1)):
                # c / a: cin -> mid (1x1x1) -> cout (3x1x1); the shortcut: 64 or cin channels -> mid
                fill(da, dtype, n, t, hw, mid, cout, (3, 1, 1), relu=relu)
                for tpool, stride in ((0, (1, 1, 1)), (1, (1, 1, 1)), (0, (1, 2, 2))):
                    fill(dc, dtype, n, t, hw, cin, mid, stride=stride, relu=relu, tpool=tpool)
                    self.answers["af_conv_ca_fusable"][self.ask("ca", show, rc, None, ra)[0]] += 1
                    fill(d1, dtype, n, t, hw, 64, mid, relu=0)
                    self.answers["af_conv_ca_fusable, projection"][self.ask("ca", show, rc, r1, ra)[0]] += 1
                # c / pool / a: the a conv reads the pooled tensor
                if t % 2 == 0:
                    fill(dc, dtype, n, t, hw, cin, mid, relu=relu, tpool=1)
                    fill(da, dtype, n, t // 2, hw, mid, cout, (3, 1, 1), relu=relu)
                    for x_sub in (0, 1, 2, 3):
                        self.answers["af_conv_cpa_fusable"][self.ask("cpa", show, rc, ra, x_sub)[0]] += 1
                # b / c: cin -> mid (1x3x3 or 3x3x3) -> cout (1x1x1)
                for kernel in ((1, 3, 3), (3, 3, 3)):
                    fill(db, dtype, n, t, hw, cin, mid, kernel, relu=relu)
                    fill(dc, dtype, n, t, hw, mid, cout, relu=relu)
                    self.answers["af_conv_bc_fusable"][self.ask("bc", show, rb, rc)[0]] += 1
            # a / b / c: cin -> inner (1x1x1 or 3x1x1) -> inner (1x3x3) -> cout, shortcut cin -> cout
            for inner32 in ("0", "1"):
                os.environ["AF_ABC_INNER32"] = inner32
                for cin, inner, cout, kta, relu, stride in itertools.product(CHANNELS[:5], CHANNELS[:4], CHANNELS[:6], (1, 3), (0, 1), STRIDES[:2]):
                    fill(da, dtype, n, t, hw, cin, inner, (kta, 1, 1), relu=relu)
                    fill(db, dtype, n, t, hw, inner, inner, (1, 3, 3), stride, relu=relu)
                    fill(dc, dtype, n, db.to, db.ho, inner, cout, relu=relu)
                    fill(d1, dtype, n, t, hw, cin, cout, stride=stride, relu=0)
                    self.answers["af_block_abc_fusable"][self.ask("abc", show, ra, rb, rc, None)[0]] += 1
                    self.answers["af_block_abc_fusable, projection"][self.ask("abc", show, ra, rb, rc, r1)[0]] += 1
            del os.environ["AF_ABC_INNER32"]


def main(parent, branch):
    for name in ("AF_FORCE_VAR", "AF_IGEMM_224", "AF_ABC_INNER32"):
        os.environ.pop(name, None)
    s = Sweep(parent, branch)
    s.layers()
    s.pairs()
    print("calls per library:", dict(s.calls), "total", sum(s.calls.values()))
    for what in sorted(s.answers):
        print("%-40s %s" % (what, dict(sorted(s.answers[what].items(), key=lambda kv: str(kv[0])))))
    thin = [name for v, name in SPECIALISED.items() if s.answers["af_conv_variant"][v] + s.answers["af_conv_variant, two segments"][v] < MIN_REACHED]
    thin += [what for what in s.answers if "fusable" in what and s.answers[what][1] < MIN_REACHED]
    for what, desc, a, b in s.different:
        print("DIFFERENT", what, desc, a, b)
    if thin:
        print("reached by fewer than %d grid points: %s" % (MIN_REACHED, thin))
    print("equal on every call" if not s.different else "%d calls differ" % sum(c["DIFFERENT"] for c in s.answers.values()))
    return 1 if s.different or thin else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
