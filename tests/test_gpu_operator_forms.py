"""GPU: both forms of every staged operator that has more than one.

Most staged operators (the C ABI entry points INTEGRATION.md maps one per reference method) choose between a vector form and an
element-wise form from a host predicate over pointer alignment, length parity, antenna shape or batch size.  Engine only ever
hands them fresh 256-byte aligned buffers, so these tests build views one element into an allocation that is one element longer
(whole elements, always inside the allocation) and walk every predicate from both sides, in both arithmetics.  Each case checks
  1. the form that ran (Engine.last_kernel(), the tags listed at mcle_ctx_last_kernel in mcle.h),
  2. the values against a plain high-precision reference (complex128: NumPy clongdouble, a few ulps scaled by the operand norms;
     complex64: a complex128 reference at ~1e-6; labels and tables exactly; Philox draws against oracle/philox.py),
  3. that the forms agree bit for bit where they keep one association.  The twin is reached by an offset pointer where one can
     reach it and otherwise through the staged_generic option.
The element beside every output view is a guard: it must keep its sentinel.
"""
import math
from ctypes import POINTER, c_double, c_void_p

import numpy as np
import pytest

from helpers import relerr
from oracle import chains, mimo as omimo, philox as P
from pyphysim_amd import _lib
from pyphysim_amd.engine import DeviceArray

pytestmark = pytest.mark.gpu

DTS = ["f32", "f64"]
CX = {"f32": np.complex64, "f64": np.complex128}
EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
PAIR = {"f32": 16, "f64": 32}                     # bytes of two complex elements
SENTINEL = {np.dtype(np.complex64): 1234.5 - 987.25j, np.dtype(np.complex128): 1234.5 - 987.25j,
            np.dtype(np.int32): -7, np.dtype(np.uint8): 0xA5}


class View:
    """A device view at element offset k of an allocation one element longer (the other element is a guard)."""

    def __init__(self, engine, shape, dtype, k=0, host=None):
        dtype = np.dtype(dtype)
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        n = int(np.prod(shape))
        self.k, self.n, self.dtype = k, n, dtype
        self.base = engine.empty(n + 1, dtype)
        self.base.set(np.full(n + 1, SENTINEL[dtype], dtype=dtype))
        v = DeviceArray.__new__(DeviceArray)
        v.engine, v.dtype, v.shape, v.size, v.nbytes = engine, dtype, shape, n, n * dtype.itemsize
        v._ptr, v._base = c_void_p(self.base.ptr.value + k * dtype.itemsize), self.base
        self.arr = v
        if host is not None:
            v.set(np.asarray(host, dtype=dtype).reshape(shape))

    @property
    def ptr(self):
        return self.arr.ptr

    @property
    def addr(self):
        return self.arr.ptr.value

    def get(self):
        full = self.base.get()
        guard = full[self.n] if self.k == 0 else full[0]
        assert guard == SENTINEL[self.dtype], "an operator wrote outside its output"
        return full[self.k:self.k + self.n].reshape(self.arr.shape)


def dtc(dt):
    return _lib.dtype_code(dt)


def crand(rs, shape, dt):
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(CX[dt])


def ld(x):
    return np.asarray(x).astype(np.clongdouble)


def assert_close(got, ref, scale, dt, c):
    """|got - ref| <= c eps scale elementwise (ref, scale in long double)."""
    err = np.abs(ld(got) - ref)
    bound = c * EPS[dt] * np.asarray(scale, dtype=np.longdouble) + np.finfo(np.float32 if dt == "f32" else np.float64).tiny
    bad = err > bound
    assert not bad.any(), "max err / bound = %g" % float(np.max(err / bound))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def with_generic(*offsets):
    """the offset cases, then None: aligned pointers under staged_generic=1"""
    return list(offsets) + [None]


def call(engine, fn, *args):
    _lib.check(getattr(engine.lib, fn)(engine.ctx, *args))


# ---- k_binary: awgn_add / cmul / cdiv -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", ["awgn", "cmul", "cdiv"])
def test_binary_forms(engine, dt, op):
    rs = np.random.RandomState(11)
    nv = 0.3
    for n in (1, 2, 7, 1000, 4097):                     # n = 1 and the odd tails: thread 0 of the pair form
        a, b = crand(rs, n, dt), crand(rs, n, dt)
        if op == "cdiv":
            b = (b + np.where(b.real >= 0, 1.0, -1.0).astype(b.dtype)).astype(CX[dt])     # away from zero
        A, B = ld(a), ld(b)
        if op == "awgn":
            s = ld(np.asarray(math.sqrt(nv), dtype=np.float32 if dt == "f32" else np.float64))
            ref, scale, c = A + s * B, np.abs(A) + np.abs(s * B), 4
        elif op == "cmul":
            ref, scale, c = A * B, np.abs(A) * np.abs(B), 4
        else:
            ref, scale, c = A / B, np.abs(A) / np.abs(B), 16   # (complex64: the fast f32 divide)
        first = None
        for offs in with_generic((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            generic = offs is None
            ka, kb, ko = offs or (0, 0, 0)
            va, vb = View(engine, n, CX[dt], ka, a), View(engine, n, CX[dt], kb, b)
            vo = View(engine, n, CX[dt], ko)
            with engine.options(staged_generic=int(generic)):
                if op == "awgn":
                    call(engine, "mcle_awgn_add", dtc(dt), va.ptr, vb.ptr, nv, vo.ptr, n)
                else:
                    call(engine, "mcle_" + op, dtc(dt), va.ptr, vb.ptr, vo.ptr, n)
                tag = engine.last_kernel()
            pair = dt == "f32" and not generic and (va.addr | vb.addr | vo.addr) % 16 == 0
            assert tag == ("binary pair" if pair else "binary elem"), (n, ka, kb, ko, generic)
            got = vo.get()
            assert_close(got, ref, scale, dt, c)
            if first is None:
                first = got
            assert same_bits(got, first), (n, ka, kb, ko, generic)
    call(engine, "mcle_cmul", dtc(dt), None, None, None, 0)
    assert engine.last_kernel() == ""                  # cleared on entry: a call that launches nothing names nothing


# ---- modulate / demodulate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_modulate_demodulate_forms(engine, dt):
    table = chains.constellation("qam", 16)
    engine.set_constellation(table, _lib.CONST_QAM)
    rs = np.random.RandomState(5)
    for n in (1, 2, 7, 1000, 1001):
        idx = rs.randint(0, 16, n).astype(np.int32)
        want = table[idx].astype(CX[dt])
        rx = (want + 0.05 * crand(rs, n, dt)).astype(CX[dt])
        mods, dems = [], []
        for offs in with_generic((0, 0), (1, 0), (0, 1), (1, 1)):
            generic = offs is None
            ki, kx = offs or (0, 0)
            vi, vo = View(engine, n, np.int32, ki, idx), View(engine, n, CX[dt], kx)
            with engine.options(staged_generic=int(generic)):
                call(engine, "mcle_modulate", dtc(dt), vi.ptr, vo.ptr, n)
                tag = engine.last_kernel()
            pair = dt == "f32" and not generic and vi.addr % 8 == 0 and vo.addr % 16 == 0
            assert tag == ("modulate pair" if pair else "modulate elem"), (n, ki, kx, generic)
            got = vo.get()
            assert np.array_equal(got, want)
            mods.append(got)
            vr, vd = View(engine, n, CX[dt], kx, rx), View(engine, n, np.int32, ki)
            with engine.options(staged_generic=int(generic)):
                call(engine, "mcle_demodulate", dtc(dt), _lib.DEMOD_MINDIST, vr.ptr, vd.ptr, n)
                tag = engine.last_kernel()
            pair = dt == "f32" and not generic and vr.addr % 16 == 0 and vd.addr % 8 == 0
            assert tag == ("demodulate pair" if pair else "demodulate elem"), (n, ki, kx, generic)
            dec = vd.get()
            assert np.array_equal(dec, idx)
            dems.append(dec)
        assert all(same_bits(m, mods[0]) for m in mods) and all(same_bits(d, dems[0]) for d in dems)


# ---- randn_c: the offset output pointer (test_philox_draws covers the parity of `first`) ---------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_randn_c_forms(engine, dt):
    seed, r, var = 20261016, 987654321, 0.25
    for first in (0, 1, 2, 7):
        for n in (1, 2, 3, 17, 1000):
            want = math.sqrt(var) * P.cnormal(seed, r, n, P.STREAM_NOISE, offset=first)
            outs = []
            for k, generic in ((0, 0), (1, 0), (0, 1)):
                vo = View(engine, n, CX[dt], k)
                with engine.options(staged_generic=generic):
                    call(engine, "mcle_randn_c", dtc(dt), seed, r, _lib.STREAM_NOISE, first, var, vo.ptr, n)
                    tag = engine.last_kernel()
                pair = dt == "f32" and not generic and first % 2 == 0 and vo.addr % 16 == 0
                assert tag == ("randn_c c64 pair" if pair else "randn_c elem"), (first, n, k, generic)
                got = vo.get()
                assert relerr(got, want) <= (1e-13 if dt == "f64" else 3e-6), (first, n, k)
                outs.append(got)
            assert all(same_bits(o, outs[0]) for o in outs), (first, n)


# ---- rand_modulate_batch (int32 and byte labels) -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("labels", [np.int32, np.uint8])
def test_rand_modulate_batch_forms(engine, dt, labels):
    table = chains.constellation("qam", 64)
    engine.set_constellation(table, _lib.CONST_QAM)
    seed, first, count = 77, (1 << 33) + 3, 2
    u8 = labels is np.uint8
    fn = "mcle_rand_modulate_batch_u8" if u8 else "mcle_rand_modulate_batch"
    for n in (1, 2, 16, 17, 32, 48, 1000):
        want = np.stack([P.symbols(seed, first + k, n, 64) for k in range(count)])
        outs = []
        for offs in with_generic((0, 0), (1, 0), (0, 1)):
            generic = offs is None
            ki, ks = offs or (0, 0)
            vi, vs = View(engine, (count, n), labels, ki), View(engine, (count, n), CX[dt], ks)
            with engine.options(staged_generic=int(generic)):
                call(engine, fn, dtc(dt), seed, first, count, vi.ptr, vs.ptr, n)
                tag = engine.last_kernel()
            if u8:
                vec = not generic and n % 16 == 0 and vi.addr % 16 == 0 and vs.addr % 16 == 0
                assert tag == ("rand_modulate_u8 x16" if vec else "rand_modulate_u8 elem"), (n, ki, ks, generic)
            else:
                vec = not generic and n % 2 == 0 and vi.addr % 8 == 0 and vs.addr % 16 == 0
                assert tag == ("rand_modulate pair" if vec else "rand_modulate elem"), (n, ki, ks, generic)
            lab, sym = vi.get(), vs.get()
            assert np.array_equal(lab, want.astype(labels))
            assert np.array_equal(sym, table[want].astype(CX[dt]))
            outs.append(sym)
        assert all(same_bits(o, outs[0]) for o in outs)


# ---- Blast encode / filter / decode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_blast_encode_forms(engine, dt):
    rs = np.random.RandomState(8)
    batch = 2
    for nt in (1, 2, 3, 4):
        for ns in (1, 6, 7, 130):
            n = nt * ns
            x = crand(rs, (batch, n), dt)
            ref = np.stack([ld(x[b]).reshape((nt, -1), order="F") / np.sqrt(np.longdouble(nt)) for b in range(batch)])
            outs = []
            for offs in with_generic((0, 0), (1, 0), (0, 1)):
                generic = offs is None
                kx, ko = offs or (0, 0)
                vx, vo = View(engine, (batch, n), CX[dt], kx, x), View(engine, (batch, nt, ns), CX[dt], ko)
                with engine.options(staged_generic=int(generic)):
                    call(engine, "mcle_blast_encode", dtc(dt), vx.ptr, nt, n, vo.ptr, batch)
                    tag = engine.last_kernel()
                pairs = (not generic and nt in (2, 4) and ns % 2 == 0 and vx.addr % PAIR[dt] == 0
                         and vo.addr % PAIR[dt] == 0)
                assert tag == ("blast_encode pairs" if pairs else "blast_encode elem"), (nt, ns, kx, ko, generic)
                got = vo.get()
                assert_close(got, ref, np.abs(ref), dt, 2)
                assert np.allclose(got, np.stack([omimo.blast_encode(x[b].astype(complex), nt) for b in range(batch)]),
                                   rtol=4 * EPS[dt], atol=0)
                outs.append(got)
            assert all(same_bits(o, outs[0]) for o in outs), (nt, ns)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nr,nt", [(4, 4), (4, 3), (3, 3), (2, 2), (2, 1)])
def test_blast_filter_forms(engine, dt, nr, nt):
    rs = np.random.RandomState(nr * 10 + nt)
    nv = 0.3
    for batch in (63, 64, 65):
        H = crand(rs, (batch, nr, nt), dt)
        ref = np.stack([omimo.blast_receive_filter(H[b].astype(complex), nv) for b in range(batch)])
        whole = (nr * nt * np.dtype(CX[dt]).itemsize) % 16 == 0
        outs = []
        for offs in with_generic((0, 0), (1, 0), (0, 1)):
            generic = offs is None
            kh, kg = offs or (0, 0)
            vh, vg = View(engine, (batch, nr, nt), CX[dt], kh, H), View(engine, (batch, nt, nr), CX[dt], kg)
            sk = View(engine, batch, np.int32, 0)
            with engine.options(staged_generic=int(generic)):
                call(engine, "mcle_blast_filter", dtc(dt), vh.ptr, nr, nt, nv, vg.ptr, sk.ptr, batch)
                tag = engine.last_kernel()
            staged = not generic and whole and (vh.addr | vg.addr) % 16 == 0 and batch >= 64
            assert tag == ("blast_filter staged" if staged else "blast_filter direct"), (batch, kh, kg, generic)
            got = vg.get()
            assert not sk.get().any()
            for b in range(batch):
                assert relerr(got[b], ref[b]) <= (1e-11 if dt == "f64" else 1e-6), (batch, b)
            outs.append(got)
        assert all(same_bits(o, outs[0]) for o in outs), batch


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nr,nt", [(4, 4), (4, 3), (3, 4), (2, 2)])
def test_blast_decode_forms(engine, dt, nr, nt):
    rs = np.random.RandomState(nr * 7 + nt)
    batch = 2
    for ns in (1, 5, 64):
        G, Y = crand(rs, (batch, nt, nr), dt), crand(rs, (batch, nr, ns), dt)
        ref = np.stack([(ld(G[b]) @ ld(Y[b])).reshape(-1, order="F") for b in range(batch)])
        scale = np.stack([(np.abs(ld(G[b])) @ np.abs(ld(Y[b]))).reshape(-1, order="F") for b in range(batch)])
        outs = []
        for offs in with_generic((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            generic = offs is None
            kg, ky, ke = offs or (0, 0, 0)
            vg, vy = View(engine, (batch, nt, nr), CX[dt], kg, G), View(engine, (batch, nr, ns), CX[dt], ky, Y)
            ve = View(engine, (batch, ns * nt), CX[dt], ke)
            with engine.options(staged_generic=int(generic)):
                call(engine, "mcle_blast_decode", dtc(dt), vg.ptr, vy.ptr, nr, nt, ns, ve.ptr, batch)
                tag = engine.last_kernel()
            if generic or (nr, nt) != (4, 4):
                want = "blast_decode generic"
            else:
                want = "blast_decode c64 4x4 x4" if dt == "f32" and ve.addr % 16 == 0 else "blast_decode 4x4"
            assert tag == want, (ns, kg, ky, ke, generic)
            got = ve.get()
            assert_close(got, ref, scale, dt, 4 * nr)
            outs.append(got)
        assert all(same_bits(o, outs[0]) for o in outs), ns


# ---- the flat MIMO channel: injected noise and on-chip noise ------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nr,nt", [(4, 4), (4, 3), (3, 4), (2, 2)])
def test_mimo_channel_forms(engine, dt, nr, nt):
    """The three k_mimo_channel forms keep one association (the cfma order, the noise after the sum): equal bits."""
    rs = np.random.RandomState(nr * 5 + nt)
    batch, nv = 2, 0.2
    sig = ld(np.asarray(math.sqrt(nv), dtype=np.float32 if dt == "f32" else np.float64))
    for ns in (1, 6, 7, 64):
        H, X, W = crand(rs, (batch, nr, nt), dt), crand(rs, (batch, nt, ns), dt), crand(rs, (batch, nr, ns), dt)
        HX = np.stack([ld(H[b]) @ ld(X[b]) for b in range(batch)])
        scale = np.stack([np.abs(ld(H[b])) @ np.abs(ld(X[b])) for b in range(batch)])
        for noisy in (False, True):
            ref = HX + sig * ld(W) if noisy else HX
            sc = scale + np.abs(sig * ld(W)) if noisy else scale
            outs = []
            for offs in with_generic((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
                generic = offs is None
                kh, kx, kw, ky = offs or (0, 0, 0, 0)
                if kw and not noisy:
                    continue
                vh, vx = View(engine, (batch, nr, nt), CX[dt], kh, H), View(engine, (batch, nt, ns), CX[dt], kx, X)
                vw = View(engine, (batch, nr, ns), CX[dt], kw, W) if noisy else None
                vy = View(engine, (batch, nr, ns), CX[dt], ky)
                with engine.options(staged_generic=int(generic)):
                    call(engine, "mcle_mimo_channel", dtc(dt), vh.ptr, vx.ptr, vw.ptr if noisy else None,
                         nv if noisy else 0.0, nr, nt, ns, vy.ptr, batch)
                    tag = engine.last_kernel()
                four = not generic and (nr, nt) == (4, 4)
                pair = four and dt == "f32" and ns % 2 == 0 and (vx.addr | vy.addr | (vw.addr if noisy else 0)) % 16 == 0
                want = "mimo_channel c64 4x4 pair" if pair else "mimo_channel 4x4" if four else "mimo_channel generic"
                assert tag == want, (ns, noisy, kh, kx, kw, ky, generic)
                got = vy.get()
                assert_close(got, ref, sc, dt, 4 * nt)
                outs.append(got)
            assert all(same_bits(o, outs[0]) for o in outs), (ns, noisy)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nr,nt", [(4, 4), (4, 3), (3, 4), (2, 2)])
def test_mimo_channel_philox_forms(engine, dt, nr, nt):
    """Y = H X + sigma CN(0,1) (NOISE stream, sample r ns + c).  The reference noise is randn_c_batch's draws of the same
    stream (checked against oracle/philox.py), so a lane-exchange or word-pairing slip is an O(1) error, not an ulp.
    complex128: the 4x4 lane form equals the generic loop bit for bit (sum first, then the noise, in both).  complex64: the
    4x4 pair form starts its sums from the noise, the generic loop adds the noise last, so those two are held to the
    tolerance instead; the generic loop reached by an offset pointer and by staged_generic are one kernel path: equal bits."""
    rs = np.random.RandomState(nr * 3 + nt)
    batch, nv, seed, first = 3, 0.3, 4242, (1 << 32) + 17
    for ns in (1, 2, 6, 7, 1040):
        H, X = crand(rs, (batch, nr, nt), dt), crand(rs, (batch, nt, ns), dt)
        z = engine.randn_c_batch(nr * ns, seed, first, batch, _lib.STREAM_NOISE, variance=nv, dtype=dt).get()
        assert relerr(z[0], math.sqrt(nv) * P.cnormal(seed, first, nr * ns, P.STREAM_NOISE)) <= \
            (1e-13 if dt == "f64" else 3e-6)
        Z = ld(z.reshape(batch, nr, ns))
        ref = np.stack([ld(H[b]) @ ld(X[b]) for b in range(batch)]) + Z
        sc = np.stack([np.abs(ld(H[b])) @ np.abs(ld(X[b])) for b in range(batch)]) + np.abs(Z)
        got_by = {}
        for offs in with_generic((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            generic = offs is None
            kh, kx, ky = offs or (0, 0, 0)
            vh, vx = View(engine, (batch, nr, nt), CX[dt], kh, H), View(engine, (batch, nt, ns), CX[dt], kx, X)
            vy = View(engine, (batch, nr, ns), CX[dt], ky)
            with engine.options(staged_generic=int(generic)):
                call(engine, "mcle_mimo_channel_philox", dtc(dt), vh.ptr, vx.ptr, seed, first, nv, nr, nt, ns, vy.ptr, batch)
                tag = engine.last_kernel()
            fast = not generic and (nr, nt) == (4, 4) and ns % 2 == 0 and (vx.addr | vy.addr) % 16 == 0
            want = ("mimo_channel_philox generic" if not fast else
                    "mimo_channel_philox c64 4x4 pair" if dt == "f32" else "mimo_channel_philox f64 4x4 lane")
            assert tag == want, (ns, kh, kx, ky, generic)
            got = vy.get()
            assert_close(got, ref, sc, dt, 4 * nt + 4)
            got_by.setdefault(want, []).append(got)
        for outs in got_by.values():
            assert all(same_bits(o, outs[0]) for o in outs), ns
        if dt == "f64":
            allv = [o for outs in got_by.values() for o in outs]
            assert all(same_bits(o, allv[0]) for o in allv), ns


# ---- Alamouti decode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_alamouti_decode_forms(engine, dt):
    rs = np.random.RandomState(21)
    batch = 2
    for nr in (1, 2, 3):
        for n in (2, 10, 64):
            H, Y = crand(rs, (batch, nr, 2), dt), crand(rs, (batch, nr, n), dt)
            refs, scales = [], []
            for b in range(batch):
                h, y = ld(H[b]), ld(Y[b])
                fro2 = np.sum(np.abs(h) ** 2)
                r = np.empty(n, dtype=np.clongdouble)
                r[0::2] = h[:, 0].conj() @ y[:, 0::2] + h[:, 1] @ y[:, 1::2].conj()
                r[1::2] = h[:, 1].conj() @ y[:, 0::2] - h[:, 0] @ y[:, 1::2].conj()
                refs.append(r / fro2 * np.sqrt(np.longdouble(2)))
                s = np.empty(n, dtype=np.longdouble)
                s[0::2] = np.abs(h[:, 0]) @ np.abs(y[:, 0::2]) + np.abs(h[:, 1]) @ np.abs(y[:, 1::2])
                s[1::2] = np.abs(h[:, 1]) @ np.abs(y[:, 0::2]) + np.abs(h[:, 0]) @ np.abs(y[:, 1::2])
                scales.append(s / fro2 * np.sqrt(np.longdouble(2)))
                assert np.allclose(omimo.alamouti_decode(Y[b].astype(complex), H[b].astype(complex)),
                                   refs[-1].astype(complex), rtol=1e-5 if dt == "f32" else 1e-12, atol=1e-6)
            ref, scale = np.stack(refs), np.stack(scales)
            outs = []
            for offs in with_generic((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                generic = offs is None
                kh, ky, ko = offs or (0, 0, 0)
                vh, vy = View(engine, (batch, nr, 2), CX[dt], kh, H), View(engine, (batch, nr, n), CX[dt], ky, Y)
                vo = View(engine, (batch, n), CX[dt], ko)
                with engine.options(staged_generic=int(generic)):
                    call(engine, "mcle_alamouti_decode", dtc(dt), vh.ptr, vy.ptr, nr, n, vo.ptr, batch)
                    tag = engine.last_kernel()
                pair = not generic and vy.addr % PAIR[dt] == 0 and vo.addr % PAIR[dt] == 0
                assert tag == ("alamouti_decode pair" if pair else "alamouti_decode elem"), (nr, n, kh, ky, ko, generic)
                got = vo.get()
                assert_close(got, ref, scale, dt, 8 * nr + 8)
                outs.append(got)
            assert all(same_bits(o, outs[0]) for o in outs), (nr, n)


# ---- Jakes taps with on-chip phases: the complex64 runs of four ---------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_jakes_taps_philox_forms(engine, dt):
    from oracle import channels as och
    seed, first, count, L, S = 31, 5, 2, 8, 3
    amp = np.linspace(0.3, 1.0, S)
    Ts, Fd = 1e-5, 120.0
    for n in (1, 3, 8, 200, 201):
        t, _ = och.jakes_time_axis(Ts, Ts, n)
        step = float(t[1] - t[0]) if n > 1 else Ts
        want = []
        for r in range(count):
            phi, psi = chains._jakes_phases(chains.PhiloxRng(seed, first + r), L, (S,))
            want.append(och.jakes_samples(phi, psi, Fd, t) * math.sqrt(L) * amp[:, None])
        outs = []
        for k, generic in ((0, 0), (1, 0), (0, 1)):
            vo = View(engine, (count, S, n), CX[dt], k)
            with engine.options(staged_generic=generic):
                call(engine, "mcle_jakes_taps_philox", dtc(dt), seed, first, count, L, S, Fd, Ts, step,
                     amp.ctypes.data_as(POINTER(c_double)), vo.ptr, n)
                tag = engine.last_kernel()
            vec = dt == "f32" and not generic and n % 2 == 0 and vo.addr % 16 == 0
            assert tag == ("jakes_taps c64 x4" if vec else "jakes_taps elem"), (n, k, generic)
            got = vo.get()
            for r in range(count):
                assert relerr(got[r], want[r]) <= (1e-10 if dt == "f64" else 3e-5), (n, k, r)
            outs.append(got)
        assert all(same_bits(o, outs[0]) for o in outs), n


def test_staged_generic_option_range(engine):
    with pytest.raises(_lib.McleError):
        engine.set_option("staged_generic", 2)
    assert engine.get_option("staged_generic") == 0
