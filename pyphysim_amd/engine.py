"""Engine: one libmcle context (one GPU, one stream) with device arrays and typed wrappers.

Everything here is plumbing around the C ABI (include/mcle.h); the arithmetic runs in the HIP
kernels under pyphysim_amd/csrc.  NumPy arrays passed to an operator are copied to the device
and the result is copied back (drop-in behaviour, PCIe-bound); :class:`DeviceArray` arguments
stay resident and results come back as DeviceArray.
"""
import contextlib
import ctypes
import math
from ctypes import byref, c_double, c_float, c_int, c_int32, c_void_p

import numpy as np

from . import _lib
from ._lib import (CONST_BPSK, CONST_GENERIC, CONST_QAM, DEMOD_MINDIST, DEMOD_QAM_SLICER, MCLE_F32, MCLE_F64,
                   AwgnCfg, Counters, FlatCfg, IaCfg, LegacySeg, McleError, MimoOfdmCfg, OfdmTdlCfg, check)


class DeviceArray:
    """A typed, shaped view of device memory owned by an Engine."""

    def __init__(self, engine, shape, dtype):
        self.engine = engine
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.size = int(np.prod(self.shape)) if self.shape else 1
        self.nbytes = self.size * self.dtype.itemsize
        self._ptr = c_void_p(0)
        if self.nbytes:
            self._ptr = engine._alloc(self.nbytes)

    @property
    def ptr(self):
        return self._ptr

    def reshape(self, *shape):
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        view = DeviceArray.__new__(DeviceArray)
        view.engine, view.dtype, view.size, view.nbytes = self.engine, self.dtype, self.size, self.nbytes
        shape = [int(v) for v in shape]
        if shape.count(-1) > 1:
            raise ValueError("can only specify one unknown dimension")
        if -1 in shape:
            known = int(np.prod([v for v in shape if v != -1])) if len(shape) > 1 else 1
            if known == 0 or self.size % known:
                raise ValueError("cannot reshape array of size %d into shape %s" % (self.size, tuple(shape)))
            shape[shape.index(-1)] = self.size // known
        if int(np.prod(shape)) != self.size:
            raise ValueError("cannot reshape array of size %d into shape %s" % (self.size, tuple(shape)))
        view.shape = tuple(shape)
        view._ptr, view._base = self._ptr, self
        return view

    def get(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            check(self.engine.lib.mcle_memcpy_d2h(self.engine.ctx, out.ctypes.data_as(c_void_p), self._ptr,
                                                  self.nbytes))
        return out

    def set(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.size != self.size:
            raise ValueError("size mismatch: %d vs %d" % (host.size, self.size))
        if self.nbytes:
            check(self.engine.lib.mcle_memcpy_h2d(self.engine.ctx, self._ptr, host.ctypes.data_as(c_void_p),
                                                  self.nbytes))
        return self

    def zero(self):
        if self.nbytes:
            check(self.engine.lib.mcle_memset(self.engine.ctx, self._ptr, 0, self.nbytes))
        return self

    def __del__(self):
        try:
            if getattr(self, "_base", None) is None and self._ptr and self._ptr.value and self.engine.ctx:
                self.engine._release(self._ptr, self.nbytes)
                self._ptr = c_void_p(0)
        except Exception:
            pass


class Engine:
    """One context on one MI355X.  ``dtype`` ('f64' parity / 'f32' throughput) is the default
    arithmetic of the operator calls; every call can override it."""

    def __init__(self, device=0, dtype="f64"):
        self.lib = _lib.load()
        self.ctx = c_void_p(0)
        self.dtype = _lib.dtype_code(dtype)
        ctx = c_void_p(0)
        check(self.lib.mcle_ctx_create(int(device), byref(ctx)))
        self.ctx = ctx
        self.device = int(device)
        self.M = 0
        self._table_key = None
        # size-keyed free list: operator calls allocate their outputs, and hipMalloc / hipFree of large
        # buffers cost far more than the kernels; all work is on one stream, so reuse is stream-ordered
        self._pool, self._pool_bytes, self.pool_limit = {}, 0, 8 << 30
        n_cu, lds = c_int(0), c_int(0)
        name = ctypes.create_string_buffer(128)
        check(self.lib.mcle_ctx_device_info(self.ctx, byref(n_cu), byref(lds), name, 128))
        self.n_cu, self.device_name = n_cu.value, name.value.decode()

    def device_info(self):
        """{'n_cu': compute units, 'name': device name} of this engine's device."""
        return {"n_cu": self.n_cu, "name": self.device_name}

    def _alloc(self, nbytes):
        free = self._pool.get(nbytes)
        if free:
            self._pool_bytes -= nbytes
            return free.pop()
        ptr = c_void_p(0)
        rc = self.lib.mcle_malloc(self.ctx, nbytes, byref(ptr))
        if rc and self._pool_bytes:
            self.empty_pool()
            rc = self.lib.mcle_malloc(self.ctx, nbytes, byref(ptr))
        check(rc)
        return ptr

    def _release(self, ptr, nbytes):
        if self._pool_bytes + nbytes <= self.pool_limit:
            self._pool.setdefault(nbytes, []).append(ptr)
            self._pool_bytes += nbytes
        else:
            self.lib.mcle_free(self.ctx, ptr)

    def last_kernel(self):
        """Diagnostic: the tag of the kernel that served this engine's last config-3 / f1 / config-4 call (run_ofdm_tdl,
        run_mimo_ofdm_tdl, run_mimo_ofdm), e.g. 'siso_wave N=1024 K=6', 'mimo_coop', 'mimo_ofdm_pw<4>/freq' or
        'mimo_ofdm_planar<1024,4,4> f32 ah4 w4 v4', or the form of the last staged operator that has more than one (the grammar:
        include/mcle.h at mcle_ctx_last_kernel); '' before such a call and after a refused one."""
        buf = ctypes.create_string_buffer(64)
        check(self.lib.mcle_ctx_last_kernel(self.ctx, buf, 64))
        return buf.value.decode()

    def empty_pool(self):
        """Returns the pooled device buffers and the context's scratch buffer (the record buffers of the two-launch
        pipelines, up to 138-320 MiB) to the allocator."""
        for free in self._pool.values():
            for ptr in free:
                self.lib.mcle_free(self.ctx, ptr)
        self._pool, self._pool_bytes = {}, 0
        check(self.lib.mcle_ctx_trim_scratch(self.ctx))

    def close(self):
        if self.ctx:
            self.empty_pool()
            self.lib.mcle_ctx_destroy(self.ctx)
            self.ctx = c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing ---------------------------------------------------------------------------
    def sync(self):
        check(self.lib.mcle_ctx_sync(self.ctx))

    # ---- kernel-selection options (mcle_ctx_set_option: per context, never read from the environment) ----
    def set_option(self, name, value):
        """name: a key of _lib.OPTIONS ('no_mfma', 'mfma_variant', 'grid_oversub', 'flat_wgs_per_cu', 'single_tdl',
        'tdl_mfma_waves', 'jakes_direct', 'f64_generic', 'f64_threads', 'bd_runtime_solve', 'demod_nocert', 'f64_variant', 'f32_mfma', 'tdl_kernel', 'mimo_tdl_kernel', 'walk_legacy', 'staged_generic', 'codebook_no_pack':
        include/mcle.h MCLE_OPT_* says what each selects); 0 restores the default."""
        if name not in _lib.OPTIONS:
            raise ValueError("unknown option %r (known: %s)" % (name, ", ".join(sorted(_lib.OPTIONS))))
        check(self.lib.mcle_ctx_set_option(self.ctx, _lib.OPTIONS[name], int(value)))

    def get_option(self, name):
        if name not in _lib.OPTIONS:
            raise ValueError("unknown option %r" % (name,))
        v = ctypes.c_longlong(0)
        check(self.lib.mcle_ctx_get_option(self.ctx, _lib.OPTIONS[name], byref(v)))
        return int(v.value)

    @contextlib.contextmanager
    def options(self, **kw):
        """with eng.options(no_mfma=1): ...  -- sets the options for the block and restores the previous values."""
        old = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)

    def use_stream(self, hip_stream_handle):
        """Adopt an external hipStream_t, e.g. ``torch.cuda.current_stream().cuda_stream``."""
        check(self.lib.mcle_ctx_set_stream(self.ctx, c_void_p(int(hip_stream_handle) if hip_stream_handle else 0)))

    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def zeros(self, shape, dtype):
        return DeviceArray(self, shape, dtype).zero()

    def to_device(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=dtype)
        return DeviceArray(self, host.shape, host.dtype).set(host)

    HBM_KINDS = {"copy": 0, "read": 1, "triad": 2, "write": 3}

    def hbm_stream_rate(self, kind="copy", nbytes=1 << 30, reps=10, blocks_per_cu=8, nontemporal=False, unroll8=False):
        """GB/s (bytes read + written per second) of the library's 16-byte streaming kernel over arrays of `nbytes` bytes:
        what this box's HBM delivers (mcle_hbm_stream_rate, csrc/kernels_hbm.hip)."""
        g = ctypes.c_double(0.0)
        check(self.lib.mcle_hbm_stream_rate(self.ctx, self.HBM_KINDS[kind] | (4 if nontemporal else 0) | (8 if unroll8 else 0), int(nbytes), int(reps), int(blocks_per_cu), byref(g)))
        return float(g.value)

    def timer_start(self):
        check(self.lib.mcle_timer_start(self.ctx))

    def timer_stop_ms(self):
        ms = c_float(0)
        check(self.lib.mcle_timer_stop_ms(self.ctx, byref(ms)))
        return ms.value

    def _dt(self, dtype):
        return self.dtype if dtype is None else _lib.dtype_code(dtype)

    def _cin(self, x, dt):
        """complex input -> (DeviceArray, was_host)"""
        if isinstance(x, DeviceArray):
            if x.dtype != np.dtype(_lib.np_complex(dt)):
                raise TypeError("device array is %s but the call runs in %s" % (x.dtype, _lib.np_complex(dt)))
            return x, False
        return self.to_device(np.asarray(x), _lib.np_complex(dt)), True

    def _iin(self, x):
        if isinstance(x, DeviceArray):
            if x.dtype != np.dtype(np.int32):
                raise TypeError("index device arrays must be int32")
            return x, False
        return self.to_device(np.asarray(x), np.int32), True

    @staticmethod
    def _out(arr, host, as_dtype=None):
        if not host:
            return arr
        res = arr.get()
        return res.astype(as_dtype) if as_dtype is not None else res

    # ---- constellation ----------------------------------------------------------------------
    def set_constellation(self, symbols, kind=CONST_GENERIC):
        symbols = np.ascontiguousarray(symbols, dtype=np.complex128).reshape(-1)
        key = (symbols.tobytes(), kind)
        if key == self._table_key:
            return
        view = symbols.view(np.float64)
        check(self.lib.mcle_set_constellation(self.ctx, view.ctypes.data_as(ctypes.POINTER(c_double)),
                                              symbols.size, int(kind)))
        self._table_key, self.M = key, symbols.size

    # ---- a2/a3/a4 ---------------------------------------------------------------------------
    def modulate(self, idx, dtype=None):
        dt = self._dt(dtype)
        d_idx, host = self._iin(idx)
        out = self.empty(d_idx.shape, _lib.np_complex(dt))
        rc = self.lib.mcle_modulate(self.ctx, dt, d_idx.ptr, out.ptr, d_idx.size)
        if rc:
            msg = self.lib.mcle_last_error().decode()
            if "between 0 and 2^M" in msg:
                raise ValueError(msg)
            raise McleError(msg)
        return self._out(out, host)

    def demodulate(self, rx, method=DEMOD_MINDIST, dtype=None):
        dt = self._dt(dtype)
        d_rx, host = self._cin(rx, dt)
        out = self.empty(d_rx.shape, np.int32)
        check(self.lib.mcle_demodulate(self.ctx, dt, int(method), d_rx.ptr, out.ptr, d_rx.size))
        return self._out(out, host, np.int64)

    def count_errors(self, tx_idx, rx_idx, bits_per_symbol, n_real=1, counters=None):
        """-> (counters dict, per-realization symbol errors, per-realization bit errors); with a device-resident
        `counters` block (new_counters()) the sums are ADDED there and nothing is read back."""
        a, _ = self._iin(tx_idx)
        b, _ = self._iin(rx_idx)
        if a.size != b.size or a.size % n_real:
            raise ValueError("size mismatch")
        if counters is not None:
            check(self.lib.mcle_count_errors(self.ctx, a.ptr, b.ptr, a.size // n_real, n_real, int(bits_per_symbol),
                                             counters.ptr, None, None))
            return None
        cnt = self.zeros(1, np.dtype((np.void, ctypes.sizeof(Counters))))
        se, be = self.empty(n_real, np.uint32), self.empty(n_real, np.uint32)
        check(self.lib.mcle_count_errors(self.ctx, a.ptr, b.ptr, a.size // n_real, n_real, int(bits_per_symbol),
                                         cnt.ptr, se.ptr, be.ptr))
        return self._counters(cnt), se.get(), be.get()

    def demod_count(self, rx, tx_idx, n_real=1, method=DEMOD_MINDIST, dtype=None, counters=None):
        dt = self._dt(dtype)
        d_rx, _ = self._cin(rx, dt)
        if isinstance(tx_idx, DeviceArray) and tx_idx.dtype == np.dtype(np.uint8):     # byte labels (rand_modulate_batch)
            a, fn = tx_idx, self.lib.mcle_demod_count_u8
        else:
            a, _ = self._iin(tx_idx)
            fn = self.lib.mcle_demod_count
        if a.size != d_rx.size or a.size % n_real:
            raise ValueError("size mismatch")
        if counters is not None:
            check(fn(self.ctx, dt, int(method), d_rx.ptr, a.ptr, a.size // n_real, n_real, counters.ptr, None, None))
            return None
        cnt = self.zeros(1, np.dtype((np.void, ctypes.sizeof(Counters))))
        se, be = self.empty(n_real, np.uint32), self.empty(n_real, np.uint32)
        check(fn(self.ctx, dt, int(method), d_rx.ptr, a.ptr, a.size // n_real, n_real, cnt.ptr, se.ptr, be.ptr))
        return self._counters(cnt), se.get(), be.get()

    def _counters(self, cnt):
        raw = cnt.get().tobytes()
        return Counters.from_buffer_copy(raw).as_dict()

    # ---- a5 ---------------------------------------------------------------------------------
    def randn_c(self, n, seed, realization, stream=_lib.STREAM_NOISE, first=0, variance=1.0, dtype=None,
                device=False):
        dt = self._dt(dtype)
        out = self.empty(n, _lib.np_complex(dt))
        check(self.lib.mcle_randn_c(self.ctx, dt, int(seed), int(realization), int(stream), int(first),
                                    float(variance), out.ptr, out.size))
        return out if device else out.get()

    def rand_symbols(self, n, M, seed, realization, first=0, device=False):
        out = self.empty(n, np.int32)
        check(self.lib.mcle_rand_symbols(self.ctx, int(seed), int(realization), int(first), int(M), out.ptr,
                                         out.size))
        return out if device else out.get().astype(np.int64)

    def awgn_add(self, x, noise, noise_var, dtype=None):
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        d_n, _ = self._cin(noise, dt)
        if d_x.size != d_n.size:
            raise ValueError("size mismatch")
        out = self.empty(d_x.shape, _lib.np_complex(dt))
        check(self.lib.mcle_awgn_add(self.ctx, dt, d_x.ptr, d_n.ptr, float(noise_var), out.ptr, d_x.size))
        return self._out(out, host)

    def cmul(self, a, b, dtype=None):
        dt = self._dt(dtype)
        d_a, host = self._cin(a, dt)
        d_b, _ = self._cin(b, dt)
        if d_a.size != d_b.size:
            raise ValueError("size mismatch")
        out = self.empty(d_a.shape, _lib.np_complex(dt))
        check(self.lib.mcle_cmul(self.ctx, dt, d_a.ptr, d_b.ptr, out.ptr, d_a.size))
        return self._out(out, host)

    def cdiv(self, num, den, dtype=None):
        dt = self._dt(dtype)
        a, host = self._cin(num, dt)
        b, _ = self._cin(den, dt)
        if a.size != b.size:
            raise ValueError("size mismatch")
        out = self.empty(a.shape, _lib.np_complex(dt))
        check(self.lib.mcle_cdiv(self.ctx, dt, a.ptr, b.ptr, out.ptr, a.size))
        return self._out(out, host)

    # ---- a6/a9 ------------------------------------------------------------------------------
    def jakes_generate(self, phi, psi, Fd, t0, dt_step, n_samples, tap_power=None, dtype=None, device=False,
                       times=None):
        """phi, psi: [L, n_streams]; returns h [n_streams, n_samples] at t0 + k*dt_step, or at the explicit
        sample times `times` (float64 [n_samples])."""
        dt = self._dt(dtype)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        psi = np.ascontiguousarray(psi, dtype=np.float64)
        L, S = phi.shape
        out = self.empty((S, n_samples), _lib.np_complex(dt))
        pw = None
        if tap_power is not None:
            pw_arr = np.ascontiguousarray(tap_power, dtype=np.float64)
            pw = pw_arr.ctypes.data_as(ctypes.POINTER(c_double))
        dp = ctypes.POINTER(c_double)
        if times is not None:
            tt = np.ascontiguousarray(times, dtype=np.float64)
            if tt.size != n_samples:
                raise ValueError("times must have n_samples entries")
            check(self.lib.mcle_jakes_generate_at(self.ctx, dt, phi.ctypes.data_as(dp), psi.ctypes.data_as(dp), L, S,
                                                  float(Fd), tt.ctypes.data_as(dp), pw, out.ptr, int(n_samples)))
        else:
            check(self.lib.mcle_jakes_generate(self.ctx, dt, phi.ctypes.data_as(dp), psi.ctypes.data_as(dp), L, S,
                                               float(Fd), float(t0), float(dt_step), pw, out.ptr, int(n_samples)))
        return out if device else out.get()

    def tdl_apply(self, x, taps, delays, dtype=None):
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        d_g, _ = self._cin(taps, dt)
        delays = np.ascontiguousarray(delays, dtype=np.int32)
        n = d_x.size
        if d_g.size != n * delays.size:
            raise ValueError("taps must be [n_taps, n]")
        out = self.empty(n + int(delays[-1]), _lib.np_complex(dt))
        check(self.lib.mcle_tdl_apply(self.ctx, dt, d_x.ptr, d_g.ptr, delays.ctypes.data_as(ctypes.POINTER(c_int32)),
                                      delays.size, out.ptr, n))
        return self._out(out, host)

    def tdl_apply_mimo(self, x, taps, delays, dtype=None):
        """x [nt, n], taps [S, nr, nt, n] -> y [nr, n + max delay] (fading.py:1107-1117)."""
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        d_g, _ = self._cin(taps, dt)
        delays = np.ascontiguousarray(delays, dtype=np.int32)
        batched = len(d_g.shape) == 5            # [batch, S, nr, nt, n] with x [batch, nt, n]
        b = d_g.shape[0] if batched else 1
        S, nr, nt, n = d_g.shape[-4:]
        if tuple(d_x.shape[-2:]) != (nt, n) or S != delays.size or d_x.size != b * nt * n:
            raise ValueError("x must be [nt, n] and taps [n_taps, nr, nt, n]")
        shape = (nr, n + int(delays.max()))
        out = self.empty(((b,) + shape) if batched else shape, _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_tdl_apply_mimo(self.ctx, dt, d_x.ptr, d_g.ptr,
                                                       delays.ctypes.data_as(ctypes.POINTER(c_int32)), S, nr, nt,
                                                       out.ptr, n, b))
        return self._out(out, host)

    def tdl_mean_freq_response(self, taps, delays, n_sym, fft_size, cp_size, num_used, dtype=None, group=None,
                               batch=None):
        """taps [S, *links, n_sym*(fft+cp)] -> H [n_sym, num_used, *links] on the used subcarriers; with
        ``group=g`` instead: taps [S, *links, n_sym*g] -> H [n_sym, fft_size, *links], all bins in natural
        order, each averaged over g consecutive samples (g = 1: per-sample response)."""
        dt = self._dt(dtype)
        d_g, host = self._cin(taps, dt)
        delays = np.ascontiguousarray(delays, dtype=np.int32)
        links = d_g.shape[1:-1] if batch is None else d_g.shape[2:-1]   # batch: taps [batch, S, *links, n]
        P = int(np.prod(links)) if links else 1
        if group is not None:
            num_used, cp_size = -int(group), 0
        shape = (n_sym, fft_size if group is not None else num_used) + tuple(links)
        out = self.empty(shape if batch is None else (batch,) + shape, _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_tdl_mean_freq_response(
            self.ctx, dt, d_g.ptr, delays.ctypes.data_as(ctypes.POINTER(c_int32)), delays.size, P, n_sym, fft_size,
            cp_size, num_used, out.ptr, 1 if batch is None else int(batch)))
        return self._out(out, host)

    def jakes_taps_philox(self, seed, first, count, L, Fd, t0, dt_step, stream_amp, n_samples, dtype=None):
        """Device-resident Jakes taps [count, n_streams, n_samples] with the phases of realization first + r
        drawn on-chip (PHASE stream); stream_amp[s] = sqrt(tap power / L)."""
        dt = self._dt(dtype)
        amp = np.ascontiguousarray(stream_amp, dtype=np.float64)
        out = self.empty((count, amp.size, n_samples), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_jakes_taps_philox(
            self.ctx, dt, int(seed), int(first), int(count), int(L), amp.size, float(Fd), float(t0), float(dt_step),
            amp.ctypes.data_as(ctypes.POINTER(c_double)), out.ptr, int(n_samples)))
        return out

    def awgn_philox(self, x, seed, first, count, noise_var, dtype=None):
        """x [count, ...] (device or host) + sqrt(noise_var) * CN(0,1) of (seed, first + r, NOISE), row-major."""
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        out = self.empty(d_x.shape, _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_awgn_philox(self.ctx, dt, d_x.ptr, int(seed), int(first), int(count),
                                                    d_x.size // max(int(count), 1), float(noise_var), out.ptr))
        return self._out(out, host)

    def rand_symbols_batch(self, n, M, seed, first, count):
        """Device int32 [count, n]: symbol i of realization first + r."""
        out = self.empty((count, n), np.int32)
        self._raise_value(self.lib.mcle_rand_symbols_batch(self.ctx, int(seed), int(first), int(count), int(M),
                                                           out.ptr, int(n)))
        return out

    def rand_modulate_batch(self, n, seed, first, count, dtype=None, labels=np.int32):
        """(labels [count, n], samples [count, n]) of realizations first .. first + count - 1 for the bound
        constellation: rand_symbols_batch and modulate in one pass over HBM.  labels: np.int32 (default) or np.uint8
        (byte labels, M <= 256: a quarter of the label traffic; demod_count takes either)."""
        dt = self._dt(dtype)
        labels = np.dtype(labels)
        if labels not in (np.dtype(np.int32), np.dtype(np.uint8)):
            raise ValueError("labels must be int32 or uint8")
        idx = self.empty((count, n), labels)
        sym = self.empty((count, n), _lib.np_complex(dt))
        fn = self.lib.mcle_rand_modulate_batch_u8 if labels == np.dtype(np.uint8) else self.lib.mcle_rand_modulate_batch
        self._raise_value(fn(self.ctx, dt, int(seed), int(first), int(count), idx.ptr, sym.ptr, int(n)))
        return idx, sym

    def slice_rows(self, x, row_len):
        """Device copy of x[..., :row_len] (x contiguous [..., n])."""
        n = x.shape[-1]
        rows = x.size // n
        out = self.empty(tuple(x.shape[:-1]) + (row_len,), x.dtype)
        isz = np.dtype(x.dtype).itemsize
        check(self.lib.mcle_memcpy_2d(self.ctx, out.ptr, row_len * isz, x.ptr, n * isz, row_len * isz, rows))
        return out

    def blast_decode_per_subcarrier(self, G, Y, dtype=None):
        """G [ns, nt, nr], Y [nr, ns] -> est [ns*nt] with est[c*nt + a]; or batched G [b, ns, nt, nr],
        Y [b, nr, ns] -> est [b, ns*nt]."""
        dt = self._dt(dtype)
        d_G, _ = self._cin(G, dt)
        d_Y, host = self._cin(Y, dt)
        batched = len(d_G.shape) == 4
        ns, nt, nr = d_G.shape[-3:]
        b = d_G.shape[0] if batched else 1
        out = self.empty((b, ns * nt) if batched else ns * nt, _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_blast_decode_per_subcarrier(self.ctx, dt, d_G.ptr, d_Y.ptr, nr, nt, ns,
                                                                    out.ptr, b))
        return self._out(out, host)

    # ---- a10/a11 ----------------------------------------------------------------------------
    def ofdm_modulate(self, x, fft_size, cp_size, num_used, batch=1, dtype=None):
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        n_in = d_x.size // batch
        n_sym = -(-n_in // num_used)
        out = self.empty((batch, n_sym * (fft_size + cp_size)), _lib.np_complex(dt))
        rc = self.lib.mcle_ofdm_modulate(self.ctx, dt, d_x.ptr, n_in, fft_size, cp_size, num_used, out.ptr, batch)
        self._raise_value(rc)
        return self._out(out, host)

    def ofdm_demodulate(self, y, fft_size, cp_size, num_used, batch=1, dtype=None):
        dt = self._dt(dtype)
        d_y, host = self._cin(y, dt)
        n_sym = (d_y.size // batch) // (fft_size + cp_size)
        out = self.empty((batch, n_sym * num_used), _lib.np_complex(dt))
        rc = self.lib.mcle_ofdm_demodulate(self.ctx, dt, d_y.ptr, n_sym, fft_size, cp_size, num_used, out.ptr, batch)
        self._raise_value(rc)
        return self._out(out, host)

    def onetap_equalize(self, data, taps, delays, fft_size, cp_size, num_used, dtype=None):
        dt = self._dt(dtype)
        d_d, host = self._cin(data, dt)
        d_g, _ = self._cin(taps, dt)
        delays = np.ascontiguousarray(delays, dtype=np.int32)
        n_sym = d_d.size // num_used
        if d_g.size != delays.size * n_sym * (fft_size + cp_size):
            raise ValueError("taps must be [n_taps, n_sym*(fft+cp)]")
        out = self.empty(d_d.size, _lib.np_complex(dt))
        check(self.lib.mcle_onetap_equalize(self.ctx, dt, d_d.ptr, d_g.ptr,
                                            delays.ctypes.data_as(ctypes.POINTER(c_int32)), delays.size, n_sym,
                                            fft_size, cp_size, num_used, out.ptr))
        return self._out(out, host)

    def _raise_value(self, rc):
        if rc:
            msg = self.lib.mcle_last_error().decode()
            if rc == -1:
                raise ValueError(msg)
            raise McleError(msg)

    # ---- a12 --------------------------------------------------------------------------------
    def blast_encode(self, x, nt, batch=1, dtype=None):
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        n = d_x.size // batch
        out = self.empty((batch, nt, n // nt if nt else 0), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_blast_encode(self.ctx, dt, d_x.ptr, nt, n, out.ptr, batch))
        return self._out(out, host)

    def blast_filter(self, H, noise_var, dtype=None, read_skipped=True):
        """H [batch, nr, nt] -> (G [batch, nt, nr], skipped [batch]); read_skipped=False leaves the flags on the
        device (returned as a DeviceArray) and saves the blocking copy."""
        dt = self._dt(dtype)
        d_H, host = self._cin(H, dt)
        b, nr, nt = d_H.shape
        G = self.empty((b, nt, nr), _lib.np_complex(dt))
        sk = self.empty(b, np.uint32)
        self._raise_value(self.lib.mcle_blast_filter(self.ctx, dt, d_H.ptr, nr, nt, float(noise_var), G.ptr, sk.ptr,
                                                     b))
        return self._out(G, host), (sk.get() if read_skipped else sk)

    def blast_decode(self, G, Y, dtype=None):
        """G [batch, nt, nr], Y [batch, nr, ns] -> est [batch, nt*ns] (Fortran interleave)."""
        dt = self._dt(dtype)
        d_G, _ = self._cin(G, dt)
        d_Y, host = self._cin(Y, dt)
        b, nt, nr = d_G.shape
        ns = d_Y.shape[-1]
        out = self.empty((b, nt * ns), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_blast_decode(self.ctx, dt, d_G.ptr, d_Y.ptr, nr, nt, ns, out.ptr, b))
        return self._out(out, host)

    def mimo_channel(self, H, X, noise=None, noise_var=0.0, dtype=None):
        dt = self._dt(dtype)
        d_H, _ = self._cin(H, dt)
        d_X, host = self._cin(X, dt)
        b, nr, nt = d_H.shape
        ns = d_X.shape[-1]
        d_n = None
        if noise is not None:
            d_n, _ = self._cin(noise, dt)
        out = self.empty((b, nr, ns), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_mimo_channel(self.ctx, dt, d_H.ptr, d_X.ptr, d_n.ptr if d_n else None,
                                                     float(noise_var), nr, nt, ns, out.ptr, b))
        return self._out(out, host)

    def mimo_channel_philox(self, H, X, seed, first, noise_var, dtype=None):
        """Y[b] = H[b] X[b] + sqrt(noise_var) * CN(0,1) drawn on-chip (NOISE stream of realization first + b, sample
        r*ns + c): the channel operator of the staged config-4 chain in one pass."""
        dt = self._dt(dtype)
        d_H, _ = self._cin(H, dt)
        d_X, host = self._cin(X, dt)
        b, nr, nt = d_H.shape
        ns = d_X.shape[-1]
        out = self.empty((b, nr, ns), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_mimo_channel_philox(self.ctx, dt, d_H.ptr, d_X.ptr, int(seed), int(first),
                                                            float(noise_var), nr, nt, ns, out.ptr, b))
        return self._out(out, host)

    def randn_c_batch(self, n, seed, first, count, stream=_lib.STREAM_CHAN, variance=1.0, dtype=None):
        """Device complex [count, n]: CN(0, variance) sample i of (seed, first + r, stream)."""
        dt = self._dt(dtype)
        out = self.empty((count, n), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_randn_c_batch(self.ctx, dt, int(seed), int(first), int(count), int(stream),
                                                      int(n), float(variance), out.ptr))
        return out

    # ---- a13: Alamouti / MRT / SVD ----------------------------------------------------------
    def alamouti_encode(self, x, batch=1, dtype=None):
        dt = self._dt(dtype)
        d_x, host = self._cin(x, dt)
        n = d_x.size // batch
        out = self.empty((batch, 2, n), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_alamouti_encode(self.ctx, dt, d_x.ptr, n, out.ptr, batch))
        return self._out(out, host)

    def alamouti_decode(self, H, Y, dtype=None):
        """H [batch, nr, 2], Y [batch, nr, n] -> [batch, n]."""
        dt = self._dt(dtype)
        d_H, _ = self._cin(H, dt)
        d_Y, host = self._cin(Y, dt)
        b, nr, _two = d_H.shape
        n = d_Y.shape[-1]
        out = self.empty((b, n), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_alamouti_decode(self.ctx, dt, d_H.ptr, d_Y.ptr, nr, n, out.ptr, b))
        return self._out(out, host)

    def mrt_encode(self, h, x, dtype=None):
        """h [batch, nt], x [batch, n] -> [batch, nt, n]."""
        dt = self._dt(dtype)
        d_h, _ = self._cin(h, dt)
        d_x, host = self._cin(x, dt)
        b, nt = d_h.shape
        n = d_x.size // b
        out = self.empty((b, nt, n), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_mrt_encode(self.ctx, dt, d_h.ptr, d_x.ptr, nt, n, out.ptr, b))
        return self._out(out, host)

    def mrt_decode(self, h, y, dtype=None):
        dt = self._dt(dtype)
        d_h, _ = self._cin(h, dt)
        d_y, host = self._cin(y, dt)
        b, nt = d_h.shape
        n = d_y.size // b
        out = self.empty((b, n), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_mrt_decode(self.ctx, dt, d_h.ptr, d_y.ptr, nt, n, out.ptr, b))
        return self._out(out, host)

    def svd_filters(self, H, dtype=None):
        """H [batch, n, n] -> (W [batch, n, n] precoder, G [batch, n, n] receive filter, S [batch, n])."""
        dt = self._dt(dtype)
        d_H, host = self._cin(H, dt)
        b, n, _n = d_H.shape
        W, G = self.empty((b, n, n), _lib.np_complex(dt)), self.empty((b, n, n), _lib.np_complex(dt))
        S = self.empty((b, n), np.float64)
        self._raise_value(self.lib.mcle_svd_filters(self.ctx, dt, d_H.ptr, n, W.ptr, G.ptr, S.ptr, b))
        return self._out(W, host), self._out(G, host), S.get()

    def gmd_filters(self, H, noise_var=0.0, dtype=None, return_skipped=False):
        """H [batch, n, n] -> (W precoder, G receive filter, R [batch, n, n] real upper triangular); with return_skipped
        also skipped [batch] (uint32: 1 where the channel is rank deficient in the call's arithmetic and W, G, R mean
        nothing -- include/mcle.h at mcle_gmd_filters)."""
        dt = self._dt(dtype)
        d_H, host = self._cin(H, dt)
        b, n, _n = d_H.shape
        W, G = self.empty((b, n, n), _lib.np_complex(dt)), self.empty((b, n, n), _lib.np_complex(dt))
        R, sk = self.empty((b, n, n), np.float64), self.empty(b, np.uint32)
        self._raise_value(self.lib.mcle_gmd_filters(self.ctx, dt, d_H.ptr, n, float(noise_var), W.ptr, G.ptr, R.ptr,
                                                    sk.ptr, b))
        if return_skipped:
            return self._out(W, host), self._out(G, host), R.get(), sk.get()
        return self._out(W, host), self._out(G, host), R.get()

    def post_processing_sinrs(self, H, W, G_H, noise_var):
        """calc_post_processing_linear_SINRs (mimo.py:62-118), batched: H [b, nr, nt], W [b, nt, ns],
        G_H [b, ns, nr] (complex128) -> linear SINRs [b, ns]."""
        H = np.ascontiguousarray(H, dtype=np.complex128)
        W = np.ascontiguousarray(W, dtype=np.complex128)
        G = np.ascontiguousarray(G_H, dtype=np.complex128)
        b, nr, nt = H.shape
        ns = W.shape[2]
        if W.shape != (b, nt, ns) or G.shape != (b, ns, nr):
            raise ValueError("shapes must be H [b, nr, nt], W [b, nt, ns], G_H [b, ns, nr]")
        out = self.empty((b, ns), np.float64)
        dH, dW, dG = self.to_device(H), self.to_device(W), self.to_device(G)
        self._raise_value(self.lib.mcle_post_processing_sinrs(self.ctx, dH.ptr, dW.ptr, dG.ptr, float(noise_var or 0.0),
                                                              nr, nt, ns, out.ptr, b))
        return out.get()

    def mu_link_stats(self, big_H, Nr, Nt, F=None, U=None, noise_var=0.0, pe=1.0, n_ext=0, joint=False, pathloss_big=None,
                      want=("Q", "Re", "B", "sinr")):
        """MultiUserChannelMatrix(ExtInt).calc_Q / calc_JP_Q / _calc_Bkl_cov_matrix_all_l / calc_SINR / calc_JP_SINR /
        calc_cov_matrix_extint_plus_noise (channels/multiuser.py:1314-2008, :2469-2807) for a batch of channels.
        big_H [b, sum Nr, sum Nt + n_ext]; F: per user [b?, rows, Ns_k] (rows = Nt[k], or sum Nt when `joint`); U: per
        user [b?, Nr[k], Ns_k].  -> dict of per-user lists: Q[k] [b, Nr_k, Nr_k], Re[k], B[k] [b, Ns_k, Nr_k, Nr_k],
        sinr[k] [b, Ns_k]."""
        from ._lib import MuStatsCfg
        H = np.ascontiguousarray(big_H, dtype=np.complex128)
        if H.ndim == 2:
            H = H[None]
        Nr, Nt = [int(v) for v in Nr], [int(v) for v in Nt]
        K, b = len(Nr), H.shape[0]
        if K < 1 or K > 4 or len(Nt) != K or max(Nr + Nt) > 4 or min(Nr + Nt) < 1 or not 0 <= int(n_ext) <= 8:
            raise ValueError("mu_link_stats covers up to 4 users with up to 4 antennas per node and 8 external antennas")
        if H.shape[1:] != (sum(Nr), sum(Nt) + int(n_ext)):
            raise ValueError("big_H must be [sum(Nr), sum(Nt) + n_ext]")
        cfg = MuStatsCfg()
        cfg.K, cfg.n_ext, cfg.joint, cfg.noise_var, cfg.pe = K, int(n_ext), 1 if joint else 0, float(noise_var or 0.0), float(pe)
        ns = [0] * K
        Fp = np.zeros((b, K, 16, 4), dtype=np.complex128)
        Up = np.zeros((b, K, 4, 4), dtype=np.complex128)
        if F is not None:
            for k in range(K):
                Fk = np.asarray(F[k], dtype=np.complex128)
                Fk = Fk.reshape(Fk.shape[0], -1) if Fk.ndim < 3 else Fk
                rows = sum(Nt) if joint else Nt[k]
                if Fk.shape[-2] != rows or Fk.shape[-1] > 4:
                    raise ValueError("precoder of user %d must have %d rows and at most 4 streams" % (k, rows))
                ns[k] = Fk.shape[-1]
                Fp[:, k, :rows, :ns[k]] = Fk
        if U is not None:
            for k in range(K):
                Uk = np.asarray(U[k], dtype=np.complex128)
                Uk = Uk.reshape(Uk.shape[0], -1) if Uk.ndim < 3 else Uk
                if Uk.shape[-2] != Nr[k] or Uk.shape[-1] != ns[k]:
                    raise ValueError("receive filter of user %d must be [Nr, Ns] = [%d, %d]" % (k, Nr[k], ns[k]))
                Up[:, k, :Nr[k], :ns[k]] = Uk
        for k in range(K):
            cfg.nr[k], cfg.nt[k], cfg.ns[k] = Nr[k], Nt[k], ns[k]
        d_pl = None
        if pathloss_big is not None:
            pl = np.ascontiguousarray(pathloss_big, dtype=np.float64)
            if pl.shape != H.shape[1:]:
                raise ValueError("the path loss matrix must have big_H's shape")
            d_pl = self.to_device(pl)
        dQ = self.empty((b, K, 4, 4), np.complex128) if "Q" in want else None
        dRe = self.empty((b, K, 4, 4), np.complex128) if "Re" in want else None
        dB = self.empty((b, K, 4, 4, 4), np.complex128) if "B" in want else None
        dS = self.empty((b, K, 4), np.float64) if ("sinr" in want and U is not None) else None
        dH, dF = self.to_device(H), self.to_device(Fp)
        dU = self.to_device(Up) if U is not None else None
        self._raise_value(self.lib.mcle_mu_link_stats(self.ctx, byref(cfg), dH.ptr, d_pl.ptr if d_pl else None, dF.ptr,
                                                      dU.ptr if dU else None, dQ.ptr if dQ else None,
                                                      dRe.ptr if dRe else None, dB.ptr if dB else None,
                                                      dS.ptr if dS else None, b))
        out = {"ns": ns}
        if dQ:
            q = dQ.get()
            out["Q"] = [q[:, k, :Nr[k], :Nr[k]] for k in range(K)]
        if dRe:
            r = dRe.get()
            out["Re"] = [r[:, k, :Nr[k], :Nr[k]] for k in range(K)]
        if dB:
            bb = dB.get()
            out["B"] = [bb[:, k, :ns[k], :Nr[k], :Nr[k]] for k in range(K)]
        if dS:
            sv = dS.get()
            out["sinr"] = [sv[:, k, :ns[k]] for k in range(K)]
        return out

    # ---- fused pipelines --------------------------------------------------------------------
    def _run(self, fn, cfg, seed, first, count, dtype, per_realization, counters=None):
        dt = self._dt(dtype)
        cnt = counters if counters is not None else self.zeros(1, np.dtype((np.void, ctypes.sizeof(Counters))))
        se = be = None
        if per_realization:
            se, be = self.empty(count, np.uint32), self.empty(count, np.uint32)
        check(fn(self.ctx, dt, byref(cfg), int(seed), int(first), int(count), cnt.ptr,
                 se.ptr if se else None, be.ptr if be else None))
        if counters is not None:
            return None
        res = self._counters(cnt)
        if per_realization:
            return res, se.get(), be.get()
        return res

    # ---- multi-GPU exchange (csrc/comm.hip): one RCCL all-reduce of the counter blocks ----------------
    @staticmethod
    def _torch_before_rccl():
        """Load order matters in a process that has PyTorch installed: initialising RCCL through libmcle and
        importing torch AFTERWARDS ends in 'double free or corruption' at interpreter exit (measured on the box,
        scripts/experiments/rccl_exit_probe.py: torch first is clean, torch later aborts, with torch's bundled
        librccl and with /opt/rocm's alike).  So torch -- if it is there at all -- is imported before the first
        RCCL call; a host without torch (a C caller) has no second runtime to collide with."""
        import importlib.util
        try:
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except (ImportError, ValueError):
            pass

    def comm_unique_id(self):
        """128-byte RCCL id, drawn by rank 0 and handed to the other ranks by the caller (pyphysim_amd.distributed)."""
        self._torch_before_rccl()
        path = _lib.torch_rccl_path()
        check(self.lib.mcle_comm_load(path.encode() if path else None))
        buf = ctypes.create_string_buffer(128)
        check(self.lib.mcle_comm_unique_id(buf, 128))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        self._torch_before_rccl()
        path = _lib.torch_rccl_path()
        check(self.lib.mcle_comm_load(path.encode() if path else None))
        check(self.lib.mcle_comm_init(self.ctx, ctypes.c_char_p(bytes(unique_id)), int(rank), int(world)))

    def comm_destroy(self):
        check(self.lib.mcle_comm_destroy(self.ctx))

    def comm_info(self):
        r, w = ctypes.c_int(0), ctypes.c_int(1)
        check(self.lib.mcle_comm_info(self.ctx, byref(r), byref(w)))
        return r.value, w.value

    def counters_allreduce(self, cnt, n=1):
        """In place on the stream: sums of words 0..5, maxima of n_symbols / n_bits, over the ranks."""
        check(self.lib.mcle_counters_allreduce(self.ctx, cnt.ptr, int(n)))

    def allreduce_f64(self, values):
        """Sum of a small float64 vector over the ranks -> NumPy array."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        d = self.to_device(v)
        check(self.lib.mcle_allreduce_f64(self.ctx, d.ptr, v.size))
        return d.get()

    def new_counters(self):
        return self.zeros(1, np.dtype((np.void, ctypes.sizeof(Counters))))

    def read_counters(self, cnt):
        return self._counters(cnt)

    def run_awgn(self, n_symbols, noise_var, seed, first, count, method=DEMOD_MINDIST, dtype=None,
                 per_realization=False, counters=None):
        cfg = AwgnCfg(int(n_symbols), int(method), float(noise_var))
        return self._run(self.lib.mcle_run_awgn, cfg, seed, first, count, dtype, per_realization, counters)

    def run_flat_fading(self, n_symbols, noise_var, seed, first, count, Fd=100.0, Ts=1e-3, L=8,
                        rayleigh_iid=False, method=DEMOD_MINDIST, dtype=None, per_realization=False,
                        counters=None):
        cfg = FlatCfg(int(n_symbols), int(method), float(noise_var), float(Fd), float(Ts), int(L),
                      1 if rayleigh_iid else 0)
        return self._run(self.lib.mcle_run_flat_fading, cfg, seed, first, count, dtype, per_realization, counters)

    def run_ofdm_tdl(self, fft_size, cp_size, num_used, n_ofdm_sym, noise_var, tap_power, tap_delay, seed, first,
                     count, Fd=10.0, Ts=1.0 / (15e3 * 1024), L=8, method=DEMOD_MINDIST, dtype=None,
                     per_realization=False, counters=None):
        cfg = OfdmTdlCfg()
        cfg.fft_size, cfg.cp_size, cfg.num_used, cfg.n_ofdm_sym = int(fft_size), int(cp_size), int(num_used), int(
            n_ofdm_sym)
        cfg.demod_method, cfg.n_taps, cfg.L = int(method), len(tap_delay), int(L)
        cfg.noise_var, cfg.Fd, cfg.Ts = float(noise_var), float(Fd), float(Ts)
        if len(tap_delay) > _lib.MAX_TAPS or len(tap_power) != len(tap_delay):
            raise ValueError("at most %d taps; powers and delays must match" % _lib.MAX_TAPS)
        for i, (p, d) in enumerate(zip(tap_power, tap_delay)):
            cfg.tap_power[i], cfg.tap_delay[i] = float(p), int(d)
        return self._run(self.lib.mcle_run_ofdm_tdl, cfg, seed, first, count, dtype, per_realization, counters)

    def run_mimo_ofdm(self, nt, nr, fft_size, cp_size, num_used, n_ofdm_sym, noise_var, seed, first, count,
                      mmse=True, method=DEMOD_MINDIST, dtype=None, per_realization=False, counters=None):
        cfg = MimoOfdmCfg(int(nt), int(nr), int(fft_size), int(cp_size), int(num_used), int(n_ofdm_sym),
                          int(method), 1 if mmse else 0, float(noise_var))
        return self._run(self.lib.mcle_run_mimo_ofdm, cfg, seed, first, count, dtype, per_realization, counters)

    def run_mimo_flat(self, scheme, nt, nr, n_symbols, noise_var, seed, first, count, mmse=False,
                      method=DEMOD_MINDIST, dtype=None, per_realization=False, counters=None):
        """The reference's MIMO application (apps/mimo/simulate_mimo.py:68-142) fused: flat H per realization and
        one of 'blast', 'mrc', 'mrt', 'alamouti', 'svd', 'gmd'; n_symbols per layer."""
        cfg = _lib.MimoFlatCfg(_lib.MIMO_SCHEMES[scheme], int(nt), int(nr), int(n_symbols), int(method),
                               1 if mmse else 0, float(noise_var))
        return self._run(self.lib.mcle_run_mimo_flat, cfg, seed, first, count, dtype, per_realization, counters)

    def run_mimo_large(self, nt, nr, n_symbols, noise_var, seed, first, count, mmse=False, method=DEMOD_MINDIST,
                       dtype=None, per_realization=False, counters=None):
        """The flat Blast link of run_mimo_flat('blast') for large arrays: 1 <= nt <= 8, nt <= nr <= 16 (nt = 1 is the
        reference's MRC), on the matrix cores; the same draws, so up to 4 x 4 the same link as run_mimo_flat."""
        cfg = _lib.MimoLargeCfg(int(nt), int(nr), int(n_symbols), int(method), 1 if mmse else 0, 0, float(noise_var))
        return self._run(self.lib.mcle_run_mimo_large, cfg, seed, first, count, dtype, per_realization, counters)

    def run_mimo_ofdm_tdl(self, nt, nr, fft_size, cp_size, num_used, n_ofdm_sym, noise_var, tap_power, tap_delay,
                          seed, first, count, Fd=10.0, Ts=1.0 / (15e3 * 1024), L=8, mmse=True, method=DEMOD_MINDIST,
                          dtype=None, per_realization=False, counters=None):
        """Fused frequency-selective MIMO-OFDM.  Raises _lib.McleUnsupported when the Doppler is
        beyond the kernel's tap model; `simulators.MimoOfdmTdlSimulator` then runs the staged chain."""
        cfg = _lib.MimoOfdmTdlCfg()
        cfg.nt, cfg.nr, cfg.fft_size, cfg.cp_size = int(nt), int(nr), int(fft_size), int(cp_size)
        cfg.num_used, cfg.n_ofdm_sym, cfg.demod_method = int(num_used), int(n_ofdm_sym), int(method)
        cfg.mmse, cfg.n_taps, cfg.L = (1 if mmse else 0), len(tap_delay), int(L)
        cfg.noise_var, cfg.Fd, cfg.Ts = float(noise_var), float(Fd), float(Ts)
        if len(tap_delay) > _lib.MAX_TAPS or len(tap_power) != len(tap_delay):
            raise ValueError("at most %d taps; powers and delays must match" % _lib.MAX_TAPS)
        for i, (p, d) in enumerate(zip(tap_power, tap_delay)):
            cfg.tap_power[i], cfg.tap_delay[i] = float(p), int(d)
        return self._run(self.lib.mcle_run_mimo_ofdm_tdl, cfg, seed, first, count, dtype, per_realization, counters)



    def run_ia(self, n_symbols, noise_var, seed, first, count, method=DEMOD_MINDIST, dtype=None,
               per_realization=False, counters=None, solver="closed_form", max_iterations=50, relative_factor=1e-6,
               initialize_with="random"):
        """Config 5 (K = 3, 2x2, one stream per user) with the closed-form solver or one of the iterative
        ones ('alt_min', 'min_leakage', 'max_sinr'; random initial precoders).  Returns the counter dict with
        the extra keys 'sum_capacity' (+ '_sq') and 'ia_runned_iterations' (+ '_sq') = per-realization values
        summed in index order (host side), and with per_realization=True also (sym_err, bit_err, capacities,
        iterations)."""
        dt = self._dt(dtype)
        cfg = IaCfg(3, 2, 2, 1, int(n_symbols), int(method), float(noise_var), _lib.IA_SOLVERS[solver],
                    int(max_iterations), float(relative_factor), _lib.IA_INITS[initialize_with], 0)
        cnt = counters if counters is not None else self.new_counters()
        se, be = self.empty(count, np.uint32), self.empty(count, np.uint32)
        cap = self.empty(count, np.float64)
        its = self.empty(count, np.uint32)
        check(self.lib.mcle_run_ia(self.ctx, dt, byref(cfg), int(seed), int(first), int(count), cnt.ptr, se.ptr,
                                   be.ptr, cap.ptr, its.ptr))
        if counters is not None:
            return None
        res = self._counters(cnt)
        caps = cap.get()
        iterative = solver != "closed_form"
        iters = its.get().astype(np.int64) if (iterative or per_realization) else None
        if res["n_skipped"] or per_realization:
            sev = se.get()
            valid = sev != 0xFFFFFFFF
            if not valid.all():
                caps_v, iters_v = caps[valid], (iters[valid] if iters is not None else None)
            else:
                caps_v, iters_v = caps, iters
        else:                                   # nothing was skipped: no masks, no per-realization error arrays
            sev, caps_v, iters_v = None, caps, iters
        res["sum_capacity"] = float(caps_v.sum())
        res["sum_capacity_sq"] = float(np.square(caps_v).sum())     # (no BLAS: its thread pool costs more than the sum)
        res["ia_runned_iterations"] = int(iters_v.sum()) if iters_v is not None else 0
        res["ia_runned_iterations_sq"] = int(np.square(iters_v).sum()) if iters_v is not None else 0
        if per_realization:
            return res, sev, be.get(), caps, iters
        return res

    def run_ia_quantized(self, n_symbols, noise_var, seed, first, count, codebook, metric="euclidean", method=DEMOD_MINDIST,
                         dtype=None, per_realization=False, solver="max_sinr", max_iterations=120, relative_factor=1e-6,
                         initialize_with="random"):
        """Limited-feedback config 5 (mcle_run_ia_quantized; apps/ia/simple_maxsinr_quantized.py): run_ia with the solver
        seeing only the channel quantized link by link to `codebook` [C, 4] (host array or DeviceArray of the call's dtype);
        data, noise, BER and 'sum_capacity' are on the true channel, on the draws of run_ia for the same seed.  Returns what
        run_ia returns plus 'quant_dist' (+ '_sq'): the realizations' sums of their nine chosen distances, summed over the
        valid realizations; with per_realization=True also (sym_err, bit_err, capacities, iterations, index [count, 3, 3],
        dist_sum [count])."""
        dt = self._dt(dtype)
        d_cb, _ = self._cin(codebook, dt)
        if len(d_cb.shape) != 2 or d_cb.shape[1] != 4:
            raise ValueError("codebook must be [C, 4] (got %s)" % (d_cb.shape,))
        cfg = IaCfg(3, 2, 2, 1, int(n_symbols), int(method), float(noise_var), _lib.IA_SOLVERS[solver],
                    int(max_iterations), float(relative_factor), _lib.IA_INITS[initialize_with], 0)
        qcfg = _lib.QuantCfg(3, 2, 2, int(d_cb.shape[0]), int(_lib.QUANT_METRICS.get(metric, metric)))
        cnt = self.new_counters()
        se, be = self.empty(count, np.uint32), self.empty(count, np.uint32)
        cap, its = self.empty(count, np.float64), self.empty(count, np.uint32)
        dsum = self.empty(count, np.float64)
        idx = self.empty((count, 3, 3), np.int32) if per_realization else None
        self._raise_value(self.lib.mcle_run_ia_quantized(self.ctx, dt, byref(cfg), byref(qcfg), d_cb.ptr, int(seed), int(first),
                                                         int(count), cnt.ptr, se.ptr, be.ptr, cap.ptr, its.ptr,
                                                         idx.ptr if per_realization else None, dsum.ptr))
        res = self._counters(cnt)
        caps, dists, sev = cap.get(), dsum.get(), se.get()
        iters = its.get().astype(np.int64)
        valid = sev != 0xFFFFFFFF
        res["sum_capacity"] = float(caps[valid].sum())
        res["sum_capacity_sq"] = float(np.square(caps[valid]).sum())
        iterative = solver != "closed_form"
        res["ia_runned_iterations"] = int(iters[valid].sum()) if iterative else 0
        res["ia_runned_iterations_sq"] = int(np.square(iters[valid]).sum()) if iterative else 0
        res["quant_dist"] = float(dists[valid].sum())
        res["quant_dist_sq"] = float(np.square(dists[valid]).sum())
        if per_realization:
            return res, sev, be.get(), caps, iters, idx.get(), dists
        return res

    def quantize_links(self, big_H, codebook, K, Nr, Nt, metric="euclidean", dtype=None, with_dist=False):
        """my_quant_func (apps/ia/simple_maxsinr_quantized.py:113-154) on a batch (mcle_quantize_links): big_H [batch, K Nr, K Nt]
        (or one [K Nr, K Nt]), codebook [C, Nr Nt] (row = codeword).  metric 'euclidean' = calc_dist, 'chordal' =
        calc_angle_dist.  Returns (index [batch, K, K] int32, big_Hq like big_H[, dist [batch, K, K] float64]); device arrays in,
        device big_Hq out."""
        dt = self._dt(dtype)
        d_H, host = self._cin(big_H, dt)
        d_cb, _ = self._cin(codebook, dt)
        K, Nr, Nt = int(K), int(Nr), int(Nt)
        single = len(d_H.shape) == 2
        if len(d_H.shape) not in (2, 3) or tuple(d_H.shape[-2:]) != (K * Nr, K * Nt):
            raise ValueError("big_H must be [batch, K*Nr, K*Nt] (got %s)" % (d_H.shape,))
        if len(d_cb.shape) != 2 or d_cb.shape[1] != Nr * Nt:
            raise ValueError("codebook must be [C, Nr*Nt] (got %s)" % (d_cb.shape,))
        b = 1 if single else int(d_H.shape[0])
        qcfg = _lib.QuantCfg(K, Nr, Nt, int(d_cb.shape[0]), int(_lib.QUANT_METRICS.get(metric, metric)))
        idx = self.empty((b, K, K), np.int32)
        Hq = self.empty(d_H.shape, _lib.np_complex(dt))
        dist = self.empty((b, K, K), np.float64) if with_dist else None
        self._raise_value(self.lib.mcle_quantize_links(self.ctx, dt, byref(qcfg), d_H.ptr, d_cb.ptr, idx.ptr, Hq.ptr,
                                                       dist.ptr if with_dist else None, b))
        out = [idx.get(), self._out(Hq, host)] + ([dist.get()] if with_dist else [])
        if single:
            out[0] = out[0][0]
            if with_dist:
                out[2] = out[2][0]
        return tuple(out)

    # ---- indoor system level (mcle_indoor_sinr / mcle_run_indoor_drops; csrc/pipeline_indoor.hip) ----
    @staticmethod
    def _indoor_cfg(rooms_per_side, side_length, ap_decimation, model, assoc, active, n_users, wall_loss_dB, tx_power,
                    noise_power, pl_n, pl_C, dist_scale, fc_MHz, hist_bins=0, hist_lo_dB=0.0, hist_step_dB=1.0):
        return _lib.IndoorCfg(int(rooms_per_side), int(ap_decimation), int(_lib.INDOOR_MODELS.get(model, model)),
                              int(_lib.INDOOR_ASSOC.get(assoc, assoc)), int(active), int(n_users), int(hist_bins), 0,
                              float(side_length), float(wall_loss_dB), float(pl_n), float(pl_C), float(dist_scale),
                              float(fc_MHz), float(tx_power), float(noise_power), float(hist_lo_dB), float(hist_step_dB))

    def indoor_sinr(self, points, rooms_per_side, side_length, ap_decimation=1, model="metis_ps7", assoc="closest",
                    wall_loss_dB=5.0, tx_power=0.1, noise_power=1e-13, pl_n=3.76, pl_C=128.1, dist_scale=1e-3, fc_MHz=900.0,
                    dtype=None, with_assoc=False):
        """SINR in dB of every point of one floor of the METIS indoor scenario with every access point transmitting
        (mcle_indoor_sinr; apps/metis_scenarios/simulate_metis_scenario.py).  points: complex (x + 1j y, metres) of any shape, or
        real [..., 2].  model 'none' / 'general' (10 pl_n log10(d dist_scale) + pl_C dB) / 'metis_ps7'; assoc 'closest' /
        'best_channel'; powers linear.  Returns float64 of the points' shape (and the chosen AP indices with with_assoc)."""
        dt = self._dt(dtype)
        pts = np.asarray(points)
        if np.iscomplexobj(pts):
            shape = pts.shape
            xy = np.ascontiguousarray(pts, dtype=np.complex128).reshape(-1).view(np.float64)
        else:
            if pts.ndim < 1 or pts.shape[-1] != 2:
                raise ValueError("points must be complex or real [..., 2] (got %s)" % (pts.shape,))
            shape = pts.shape[:-1]
            xy = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)
        n = xy.size // 2
        cfg = self._indoor_cfg(rooms_per_side, side_length, ap_decimation, model, assoc, 0, 0, wall_loss_dB, tx_power,
                               noise_power, pl_n, pl_C, dist_scale, fc_MHz)
        d_xy = self.to_device(xy)
        sinr = self.empty(n, np.float64)
        idx = self.empty(n, np.int32) if with_assoc else None
        self._raise_value(self.lib.mcle_indoor_sinr(self.ctx, dt, byref(cfg), d_xy.ptr, n, sinr.ptr,
                                                    idx.ptr if with_assoc else None))
        out = sinr.get().reshape(shape)
        return (out, idx.get().reshape(shape)) if with_assoc else out

    def run_indoor_drops(self, rooms_per_side, side_length, ap_decimation, n_users, seed, first, count, model="metis_ps7",
                         assoc="best_channel", active=True, wall_loss_dB=5.0, tx_power=0.1, noise_power=1e-13, pl_n=3.76,
                         pl_C=128.1, dist_scale=1e-3, fc_MHz=900.0, hist_bins=0, hist_lo_dB=0.0, hist_step_dB=1.0,
                         positions=None, dtype=None, per_user=False):
        """`count` user drops on one floor of the METIS indoor scenario (mcle_run_indoor_drops;
        apps/metis_scenarios/simulate_metis_scenario2.py, one drop per call there): drop r places n_users users from the Philox
        draws of realization first + r (or at positions [count, n_users], complex or real [..., 2]), each user takes its AP,
        with `active` the APs nobody chose are switched off.  Returns a dict: 'hist' [hist_bins + 2] and 'load_hist'
        [n_users + 1] (exact integer counts), 'sum_capacity', 'sum_sinr_dB', 'min_sinr_dB', 'active_aps' [count]; with
        per_user also 'sinr_dB', 'capacity', 'assoc' [count, n_users]."""
        dt = self._dt(dtype)
        count, U = int(count), int(n_users)
        cfg = self._indoor_cfg(rooms_per_side, side_length, ap_decimation, model, assoc, bool(active), U, wall_loss_dB,
                               tx_power, noise_power, pl_n, pl_C, dist_scale, fc_MHz, hist_bins, hist_lo_dB, hist_step_dB)
        d_pos = None
        if isinstance(positions, DeviceArray):           # resident float64 [count, n_users, 2]
            if positions.dtype != np.dtype(np.float64) or positions.size != count * U * 2:
                raise ValueError("device positions must be float64 [count, n_users, 2]")
            d_pos = positions
        elif positions is not None:
            pos = np.asarray(positions)
            pos = (np.ascontiguousarray(pos, dtype=np.complex128).reshape(-1).view(np.float64) if np.iscomplexobj(pos)
                   else np.ascontiguousarray(pos, dtype=np.float64).reshape(-1))
            if pos.size != count * U * 2:
                raise ValueError("positions must hold count x n_users points (got %d values)" % pos.size)
            d_pos = self.to_device(pos)
        bins = max(int(hist_bins), 0)
        hist, load = self.zeros(bins + 2, np.uint64), self.zeros(max(U, 0) + 1, np.uint64)
        per_drop = [self.empty(count, np.float64) for _ in range(3)]
        act = self.empty(count, np.int32)
        per = [self.empty((count, max(U, 0)), t) for t in (np.float64, np.float64, np.int32)] if per_user else [None] * 3
        ptr = lambda a: a.ptr if a is not None else None
        self._raise_value(self.lib.mcle_run_indoor_drops(self.ctx, dt, byref(cfg), int(seed), int(first), count, ptr(d_pos),
                                                         hist.ptr, load.ptr, per_drop[0].ptr, per_drop[1].ptr, per_drop[2].ptr,
                                                         act.ptr, ptr(per[0]), ptr(per[1]), ptr(per[2])))
        res = dict(hist=hist.get(), load_hist=load.get(), sum_capacity=per_drop[0].get(), sum_sinr_dB=per_drop[1].get(),
                   min_sinr_dB=per_drop[2].get(), active_aps=act.get())
        if per_user:
            res.update(sinr_dB=per[0].get(), capacity=per[1].get(), assoc=per[2].get())
        return res

    # ---- hexagonal-cell system level (mcle_hex_gains / mcle_run_hex_drops; csrc/pipeline_hex.hip) ----
    @staticmethod
    def _hex_cfg(num_cells, cell_radius, users_per_cell=1, model="general", wrap_around=False, n_ext=0, min_dist_ratio=0.0,
                 pl_n=3.76, pl_C=128.1, dist_scale=1.0, tx_power=1.0, noise_power=1e-13, ext_power=0.0, hist_bins=0,
                 hist_lo_dB=0.0, hist_step_dB=1.0):
        """The config with the geometry tables of pyphysim_amd.cell; a cluster the host geometry refuses is left to the
        library's own message (its tables stay empty)."""
        from . import cell
        cfg = _lib.HexCfg()
        cfg.num_cells, cfg.users_per_cell, cfg.model = int(num_cells), int(users_per_cell), int(_lib.HEX_MODELS.get(model, model))
        cfg.wrap_around, cfg.n_ext, cfg.hist_bins = int(bool(wrap_around)), int(n_ext), int(hist_bins)
        cfg.cell_radius, cfg.min_dist_ratio = float(cell_radius), float(min_dist_ratio)
        cfg.pl_n, cfg.pl_C, cfg.dist_scale = float(pl_n), float(pl_C), float(dist_scale)
        cfg.tx_power, cfg.noise_power, cfg.ext_power = float(tx_power), float(noise_power), float(ext_power)
        cfg.hist_lo_dB, cfg.hist_step_dB = float(hist_lo_dB), float(hist_step_dB)
        K, r = int(num_cells), float(cell_radius)
        if 1 <= K <= cell.MAX_CELLS and np.isfinite(r) and r > 0 and (not wrap_around or K == 19):
            pos, start, ext_radius, centre = cell.hex_tables(K, r, bool(wrap_around))
            cfg.n_pos, cfg.external_radius = len(pos), float(ext_radius)
            cfg.centre_x, cfg.centre_y = float(centre.real), float(centre.imag)
            for i, v in enumerate(start):
                cfg.pos_start[i] = int(v)
            for i, v in enumerate(pos):
                cfg.pos_x[i], cfg.pos_y[i] = float(v.real), float(v.imag)
        return cfg

    @staticmethod
    def _points_xy(points, what="points"):
        pts = np.asarray(points)
        if np.iscomplexobj(pts):
            return pts.shape, np.ascontiguousarray(pts, dtype=np.complex128).reshape(-1).view(np.float64)
        if pts.ndim < 1 or pts.shape[-1] != 2:
            raise ValueError("%s must be complex or real [..., 2] (got %s)" % (what, pts.shape))
        return pts.shape[:-1], np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)

    def hex_gains(self, points, num_cells, cell_radius, dtype=None, **cfg):
        """Distances, gains, SINR and best cell of every point against a cluster of `num_cells` hexagonal cells
        (mcle_hex_gains; pyphysim_amd.cell.Cluster's geometry).  points: complex (x + 1j y) of any shape, or real [..., 2].
        Keywords: model 'none' / 'general' (10 pl_n log10(d dist_scale) + pl_C dB; default PathLoss3GPP1 on km),
        wrap_around (19 cells), tx_power, noise_power, ext_power (linear).  Returns a dict: 'dist' [..., K], 'gain'
        [..., K + 1] (last column: the interferer), 'sinr_dB' [...], 'assoc' [...] (first cell of the largest gain)."""
        dt = self._dt(dtype)
        shape, xy = self._points_xy(points)
        n, K = xy.size // 2, max(int(num_cells), 0)
        c = self._hex_cfg(num_cells, cell_radius, **cfg)
        d_xy = self.to_device(xy)
        dist, gain = self.empty((n, K), np.float64), self.empty((n, K + 1), np.float64)
        sinr, idx = self.empty(n, np.float64), self.empty(n, np.int32)
        self._raise_value(self.lib.mcle_hex_gains(self.ctx, dt, byref(c), d_xy.ptr, n, dist.ptr, gain.ptr, sinr.ptr, idx.ptr))
        return dict(dist=dist.get().reshape(shape + (K,)), gain=gain.get().reshape(shape + (K + 1,)),
                    sinr_dB=sinr.get().reshape(shape), assoc=idx.get().reshape(shape))

    def run_hex_drops(self, num_cells, cell_radius, users_per_cell, seed, first, count, positions=None, dtype=None,
                      per_user=False, records=False, **cfg):
        """`count` user drops in a cluster of hexagonal cells (mcle_run_hex_drops; the 'Random' user positioning of
        apps/comp_BD/simulate_comp.py): drop r places users_per_cell users at random in every cell from the Philox draws of
        realization first + r (or at positions [count, K U], complex or real [..., 2], host or resident float64
        [count, K U, 2]); every user is served by its own cell.  Keywords as for hex_gains plus min_dist_ratio, n_ext,
        hist_bins, hist_lo_dB, hist_step_dB.  Returns a dict: 'flags' [count], 'hist' [hist_bins + 2] (exact counts),
        'sum_capacity', 'min_sinr_dB' [count]; with per_user also 'positions' (complex), 'sinr_dB', 'capacity' [count, K U];
        with records=True also 'records': the RESIDENT float64 [count, K U, K + n_ext] of linear path losses -- with one user
        per cell what run_comp takes as pathloss_per_realization."""
        dt = self._dt(dtype)
        count, K, U = int(count), max(int(num_cells), 0), max(int(users_per_cell), 0)
        KU, E = K * U, max(int(cfg.get("n_ext", 0)), 0)
        c = self._hex_cfg(num_cells, cell_radius, users_per_cell, **cfg)
        d_pos = None
        if isinstance(positions, DeviceArray):
            if positions.dtype != np.dtype(np.float64) or positions.size != count * KU * 2:
                raise ValueError("device positions must be float64 [count, K U, 2]")
            d_pos = positions
        elif positions is not None:
            _, pos = self._points_xy(positions, "positions")
            if pos.size != count * KU * 2:
                raise ValueError("positions must hold count x K U points (got %d values)" % (pos.size // 2))
            d_pos = self.to_device(pos)
        hist = self.zeros(max(int(cfg.get("hist_bins", 0)), 0) + 2, np.uint64)
        flags = self.empty(count, np.int32)
        per_drop = [self.empty(count, np.float64) for _ in range(2)]
        rec = self.empty((count, KU, K + E), np.float64) if records else None
        per = ([self.empty((count, KU, 2), np.float64)] + [self.empty((count, KU), np.float64) for _ in range(2)]
               if per_user else [None] * 3)
        ptr = lambda a: a.ptr if a is not None else None
        self._raise_value(self.lib.mcle_run_hex_drops(self.ctx, dt, byref(c), int(seed), int(first), count, ptr(d_pos),
                                                      flags.ptr, ptr(rec), ptr(per[0]), ptr(per[1]), ptr(per[2]), hist.ptr,
                                                      per_drop[0].ptr, per_drop[1].ptr))
        res = dict(flags=flags.get(), hist=hist.get(), sum_capacity=per_drop[0].get(), min_sinr_dB=per_drop[1].get())
        if per_user:
            res.update(positions=np.ascontiguousarray(per[0].get()).view(np.complex128).reshape(count, KU),
                       sinr_dB=per[1].get(), capacity=per[2].get())
        if records:
            res["records"] = rec
        return res

    def ia_iterative(self, solver, big_H, F_init, noise_var, max_iterations=50, relative_factor=1e-6,
                     initialize_with="fix"):
        """IterativeIASolverBaseClass.solve (algorithms.py:802-883) with initialize_with='fix': big_H
        [batch, 6, 6], F_init [batch, 3, 2] (unit-norm initial precoders) -> dict(F, U = full_W_H, sinr,
        capacity, iterations, skipped)."""
        H = np.ascontiguousarray(big_H, dtype=np.complex128).reshape(-1, 6, 6)
        F0 = np.ascontiguousarray(F_init, dtype=np.complex128).reshape(-1, 3, 2)
        b = H.shape[0]
        if F0.shape[0] != b:
            raise ValueError("big_H and F_init must have the same batch size")
        d_H, d_F0 = self.to_device(H), self.to_device(F0)
        F, U = self.empty((b, 3, 2), np.complex128), self.empty((b, 3, 2), np.complex128)
        sinr, cap = self.empty((b, 3), np.float64), self.empty(b, np.float64)
        its, sk = self.empty(b, np.uint32), self.empty(b, np.uint32)
        self._raise_value(self.lib.mcle_ia_iterative(
            self.ctx, _lib.IA_SOLVERS[solver], _lib.IA_INITS[initialize_with], d_H.ptr, d_F0.ptr, float(noise_var),
            int(max_iterations),
            float(relative_factor), F.ptr, U.ptr, sinr.ptr, cap.ptr, its.ptr, sk.ptr, b))
        return dict(F=F.get(), U=U.get(), sinr=sinr.get(), capacity=cap.get(), iterations=its.get(),
                    skipped=sk.get())

    def ia_solve_general(self, solver, big_H, K, nr, nt, Ns, noise_var, max_iterations=50, relative_factor=1e-6,
                         F_init=None, select=None):
        """Iterative IA for general geometries (csrc/kernels_ia_general.hip; reference ia/algorithms.py:802-883,
        885-1507, 1853-2260): K <= 4 users with nr x nt <= 6 x 6 antennas, Ns = streams per user (int or list).
        big_H [batch, K nr, K nt].  Padded arrays are D x D with D = 4 when max(nr, nt) <= 4, else 6 (the library's two
        capacities).  F_init: [batch, 4, D, D] (user, nt x ns in the top-left corner; [batch, K, D, D] is padded here)
        -- 'fix' / a captured random start -- or None for the 'svd' start.  select: None, 'greedy' (GreedStreamIASolver)
        or 'brute' (BruteForceStreamIASolver, always from 'svd').  -> dict of padded arrays: F [b, K, D, D] (nt x ns in the
        top-left corner), U = full_W_H [b, K, D, D] (ns x nr), sinr [b, K, D], capacity [b], iterations [b],
        Ns [b, K], skipped [b] (+ every_capacity [b, prod(Ns)] for 'brute').  Outside the envelope (include/mcle.h: K in
        [2, 4], Nr, Nt in [1, 6], Ns[k] in [1, min(Nr, Nt)], max_iterations >= 1, noise_var >= 0, 'svd' and 'brute' with
        Nr == Nt, at most 256 stream combinations) -> ValueError and last_kernel() == ''; else 'ia_general<D> K=.. NrxNt'."""
        D = 4 if max(int(nr), int(nt)) <= 4 else 6
        H = np.ascontiguousarray(big_H, dtype=np.complex128)
        if H.ndim == 2:
            H = H[np.newaxis]
        b = H.shape[0]
        if H.shape[1:] != (K * nr, K * nt):
            raise ValueError("big_H must be [batch, K*nr, K*nt]")
        cfg = _lib.IaGeneralCfg()
        cfg.K, cfg.nr, cfg.nt = int(K), int(nr), int(nt)
        ns_list = [int(Ns)] * K if np.isscalar(Ns) else [int(n) for n in Ns]
        if len(ns_list) != K:
            raise ValueError("Ns must be an int or one value per user")
        for k in range(4):
            cfg.ns[k] = ns_list[k] if k < K else 0
        cfg.solver = _lib.IA_SOLVERS[solver]
        cfg.initialize_with = 0 if (F_init is not None and select != "brute") else 3
        cfg.max_iterations = int(max_iterations)
        cfg.stream_selection = _lib.IA_STREAM_SELECTION[select]
        cfg.noise_var, cfg.relative_factor = float(noise_var), float(relative_factor)
        d_H = self.to_device(H)
        d_F0 = None
        if cfg.initialize_with == 0:
            F0 = np.ascontiguousarray(F_init, dtype=np.complex128)
            if F0.ndim == 4 and F0.shape[0] == b and F0.shape[1] in (K, 4) and F0.shape[2] <= D and F0.shape[3] <= D:
                pad = np.zeros((b, 4, D, D), dtype=np.complex128)       # any smaller padding is re-padded to the capacity
                pad[:, :F0.shape[1], :F0.shape[2], :F0.shape[3]] = F0
                F0 = pad
            if F0.shape != (b, 4, D, D):
                raise ValueError("F_init must be [batch, 4, %d, %d] (user, nt, ns; zero padded)" % (D, D))
            d_F0 = self.to_device(F0)
        F, U = self.empty((b, 4, D, D), np.complex128), self.empty((b, 4, D, D), np.complex128)
        sinr, cap = self.empty((b, 4, D), np.float64), self.empty(b, np.float64)
        its, ns, sk = self.empty(b, np.uint32), self.empty((b, 4), np.int32), self.empty(b, np.uint32)
        every = self.empty((b, 256), np.float64) if select == "brute" else None
        self._raise_value(self.lib.mcle_ia_solve_general(self.ctx, byref(cfg), d_H.ptr, d_F0.ptr if d_F0 else None,
                                                         F.ptr, U.ptr, sinr.ptr, cap.ptr, its.ptr, ns.ptr, sk.ptr,
                                                         every.ptr if every else None, b))
        out = dict(F=F.get()[:, :K], U=U.get()[:, :K], sinr=sinr.get()[:, :K], capacity=cap.get(),
                   iterations=its.get().astype(np.int64), Ns=ns.get()[:, :K], skipped=sk.get())
        if every:
            out["every_capacity"] = every.get()[:, :int(np.prod(ns_list))]     # one value per stream combination
        return out

    def run_ia_general(self, K, nr, nt, Ns, n_symbols, noise_var, seed, first, count, solver="max_sinr", select=None,
                       initialize_with="random", max_iterations=60, relative_factor=1e-6, method=DEMOD_MINDIST, dtype=None,
                       per_realization=False, outputs=()):
        """The IA link on a general geometry, fused (csrc/pipeline_ia_general.hip, include/mcle.h at mcle_run_ia_general;
        apps/ia/simulate_ia.py with Nr, Nt, Ns as parameters, apps/ia/simulate_greedy_ia.py): K <= 4 users of nr x nt <= 6 x 6
        antennas, Ns = configured streams per user (int or one per user), solver 'alt_min' / 'min_leakage' / 'max_sinr' from a
        'random' start drawn on the device or the 'svd' start, select None / 'greedy' / 'brute' (brute force always starts
        from 'svd'); n_symbols per KEPT stream at unit power per user.
        -> the counter dict ('n_symbols' / 'n_bits': the figures with every configured stream active) with 'sum_capacity'
        (+ '_sq') and 'ia_runned_iterations' (+ '_sq') summed over the valid realizations, as run_ia; with
        per_realization=True (counters, dict(sym_err [count], bit_err [count], stream_sym_err / stream_bit_err [count, K, 6]
        by (user, kept stream), ns [count, K], capacity [count], iterations [count])).  `outputs` names what else to copy
        back into that dict: 'big_H' [count, K nr, K nt], 'F_init' / 'F' / 'U' [count, K, D, D] (the solver's padded layout,
        D = 4 while max(nr, nt) <= 4, else 6), 'sinr' [count, K, 6].  Outside the envelope -> ValueError, last_kernel() == '';
        else 'ia_general_link f64|f32 D<4|6> pairs|single'."""
        known = ("big_H", "F_init", "F", "U", "sinr")
        for name in outputs:
            if name not in known:
                raise ValueError("unknown output %r (known: %s)" % (name, ", ".join(known)))
        if outputs and not per_realization:
            raise ValueError("outputs come with per_realization=True")
        if solver not in ("alt_min", "min_leakage", "max_sinr"):
            raise ValueError("the general-geometry solvers are 'alt_min', 'min_leakage' and 'max_sinr' (got %r)" % (solver,))
        if initialize_with not in ("random", "svd"):
            raise ValueError("initialize_with must be 'random' or 'svd'")
        K, nr, nt, count = int(K), int(nr), int(nt), int(count)
        ns_list = [int(Ns)] * K if np.isscalar(Ns) else [int(n) for n in Ns]
        if len(ns_list) != K:
            raise ValueError("Ns must be an int or one value per user")
        cfg = _lib.IaGeneralCfg()
        cfg.K, cfg.nr, cfg.nt = K, nr, nt
        for k in range(4):
            cfg.ns[k] = ns_list[k] if k < K else 0
        cfg.solver = _lib.IA_SOLVERS[solver]
        cfg.initialize_with = 3 if (initialize_with == "svd" or select == "brute") else 0
        cfg.max_iterations = int(max_iterations)
        cfg.stream_selection = _lib.IA_STREAM_SELECTION[select]
        cfg.noise_var, cfg.relative_factor = float(noise_var), float(relative_factor)
        dt = self._dt(dtype)
        D = 4 if max(nr, nt) <= 4 else 6
        in_envelope = 2 <= K <= 4 and 1 <= nr <= 6 and 1 <= nt <= 6     # anything else is refused by the library below
        cnt = self.new_counters()
        se, be = self.empty(count, np.uint32), self.empty(count, np.uint32)
        ns, cap, its = self.empty((count, 4), np.int32), self.empty(count, np.float64), self.empty(count, np.uint32)
        opt = {}
        if per_realization:
            opt["stream_sym_err"] = self.empty((count, 4, 6), np.uint32)
            opt["stream_bit_err"] = self.empty((count, 4, 6), np.uint32)
            shapes = dict(big_H=(count, K * nr, K * nt), F_init=(count, 4, D, D), F=(count, 4, D, D), U=(count, 4, D, D))
            for name in outputs:
                if name == "sinr":
                    opt[name] = self.empty((count, 4, 6), np.float64)
                else:
                    opt[name] = self.empty(shapes[name] if in_envelope else (0,), np.complex128)
        ptr = lambda name: opt[name].ptr if name in opt else None
        self._raise_value(self.lib.mcle_run_ia_general(
            self.ctx, dt, byref(cfg), int(n_symbols), int(method), int(seed), int(first), count, cnt.ptr, se.ptr, be.ptr,
            ptr("stream_sym_err"), ptr("stream_bit_err"), ns.ptr, ptr("sinr"), cap.ptr, its.ptr, ptr("big_H"), ptr("F_init"),
            ptr("F"), ptr("U")))
        res = self._counters(cnt)
        sev, caps, iters = se.get(), cap.get(), its.get().astype(np.int64)
        valid = sev != 0xFFFFFFFF
        res["sum_capacity"] = float(caps[valid].sum())
        res["sum_capacity_sq"] = float(np.square(caps[valid]).sum())
        res["ia_runned_iterations"] = int(iters[valid].sum())
        res["ia_runned_iterations_sq"] = int(np.square(iters[valid]).sum())
        if not per_realization:
            return res
        out = dict(sym_err=sev, bit_err=be.get(), ns=ns.get()[:, :K], capacity=caps, iterations=iters)
        for name, arr in opt.items():
            host = arr.get()
            out[name] = host if name == "big_H" else host[:, :K]
        return res, out

    def ia_closed_form(self, big_H, noise_var):
        """big_H [batch, 6, 6] complex128 -> dict(F [batch,3,2], U [batch,3,2], sinr [batch,3],
        capacity [batch], skipped [batch])."""
        H = np.ascontiguousarray(big_H, dtype=np.complex128).reshape(-1, 6, 6)
        b = H.shape[0]
        d_H = self.to_device(H)
        F, U = self.empty((b, 3, 2), np.complex128), self.empty((b, 3, 2), np.complex128)
        sinr, cap, sk = self.empty((b, 3), np.float64), self.empty(b, np.float64), self.empty(b, np.uint32)
        check(self.lib.mcle_ia_closed_form(self.ctx, d_H.ptr, float(noise_var), F.ptr, U.ptr, sinr.ptr, cap.ptr,
                                           sk.ptr, b))
        return dict(F=F.get(), U=U.get(), sinr=sinr.get(), capacity=cap.get(), skipped=sk.get())

    # ---- block diagonalisation (comm/blockdiagonalization.py, comm/waterfilling.py) -------------
    def waterfilling(self, gains, total_power, noise_var=1.0):
        """doWF (waterfilling.py:15-92) on gains [batch, n] (or [n]) -> (powers, water levels)."""
        g = np.ascontiguousarray(gains, dtype=np.float64)
        single = g.ndim == 1
        if single:
            g = g.reshape(1, -1)
        elif g.ndim != 2:
            raise ValueError("gains must be [n] or [batch, n]")
        b, n = g.shape
        d_g = self.to_device(g)
        P, mu = self.empty((b, n), np.float64), self.empty(b, np.float64)
        self._raise_value(self.lib.mcle_waterfilling(self.ctx, d_g.ptr, n, float(total_power), float(noise_var),
                                                     P.ptr, mu.ptr, b))
        P, mu = P.get(), mu.get()
        return (P[0], float(mu[0])) if single else (P, mu)

    def block_diagonalize(self, H, num_users, iPu, noise_var, waterfilling=True):
        """BlockDiagonalizer.block_diagonalize / block_diagonalize_no_waterfilling + calc_receive_filter on
        H [batch, n, n] (n = num_users * antennas per user) -> dict(Ms, newH, W, sigma, skipped)."""
        H = np.ascontiguousarray(H, dtype=np.complex128)
        if H.ndim == 2:
            H = H[None]
        b, n, n2 = H.shape
        if n != n2 or n % int(num_users):
            raise ValueError("block diagonalisation needs a square channel whose size is a multiple of num_users")
        d_H = self.to_device(H)
        Ms, newH, W = (self.empty((b, n, n), np.complex128) for _ in range(3))
        sg, sk = self.empty((b, n), np.float64), self.empty(b, np.uint32)
        self._raise_value(self.lib.mcle_block_diagonalize(self.ctx, d_H.ptr, int(num_users), n // int(num_users),
                                                          float(iPu), float(noise_var), 1 if waterfilling else 0,
                                                          Ms.ptr, newH.ptr, W.ptr, sg.ptr, sk.ptr, b))
        return dict(Ms=Ms.get(), newH=newH.get(), W=W.get(), sigma=sg.get(), skipped=sk.get())

    def bd_extint(self, big_H, num_users, n_ant, n_ext, iPu, noise_var, pe, method="whitening", metric=None,
                  num_streams=0, ns_user=None):
        """Block diagonalisation with external interference (csrc/kernels_bd.hip k_bd_extint; reference
        comm/blockdiagonalization.py:666-1469).  big_H [batch, K r, K r + n_ext] (MultiUserChannelMatrixExtInt.big_H);
        method 'whitening' (WhiteningBD) or 'enhanced' (EnhancedBD with metric None / 'naive' / 'fixed' / 'capacity' /
        'candidates' (report the SINRs of every stream count) / 'per_user' (ns_user given)).
        -> dict(Ms [b, K, K r, r], W [b, K, r, r], Ns [b, K], cand_sinr [b, K, r, r] or None, skipped [b])."""
        H = np.ascontiguousarray(big_H, dtype=np.complex128)
        if H.ndim == 2:
            H = H[np.newaxis]
        b, n = H.shape[0], num_users * n_ant
        if H.shape[1:] != (n, n + n_ext):
            raise ValueError("big_H must be [batch, K*r, K*r + n_ext]")
        cfg = _lib.BdExtIntCfg()
        cfg.num_users, cfg.n_ant_per_user, cfg.n_ext = int(num_users), int(n_ant), int(n_ext)
        cfg.method = {"whitening": 0, "enhanced": 1}[method]
        cfg.metric = _lib.BD_METRICS[metric]
        cfg.num_streams = int(num_streams or 0)
        for k in range(4):
            cfg.ns_user[k] = int(ns_user[k]) if (ns_user is not None and k < len(ns_user)) else 0
        cfg.iPu, cfg.noise_var, cfg.pe = float(iPu), float(noise_var or 0.0), float(pe)
        d_H = self.to_device(H)
        Ms, W = self.empty((b, num_users, n, n_ant), np.complex128), self.empty((b, num_users, n_ant, n_ant), np.complex128)
        ns, sk = self.empty((b, num_users), np.int32), self.empty(b, np.uint32)
        cand = self.empty((b, num_users, n_ant, n_ant), np.float64) if cfg.metric == 4 else None
        self._raise_value(self.lib.mcle_bd_extint(self.ctx, byref(cfg), d_H.ptr, Ms.ptr, W.ptr, ns.ptr,
                                                  cand.ptr if cand is not None else None, sk.ptr, b))
        return dict(Ms=Ms.get(), W=W.get(), Ns=ns.get(), cand_sinr=None if cand is None else cand.get(),
                    skipped=sk.get())

    def pinv(self, A, rcond=1e-15):
        """np.linalg.pinv for small matrices [batch, m, n] (or [m, n]), m, n <= 8."""
        A = np.ascontiguousarray(A, dtype=np.complex128)
        single = A.ndim == 2
        if single:
            A = A[None]
        b, m, n = A.shape
        d_A, out = self.to_device(A), self.empty((b, n, m), np.complex128)
        self._raise_value(self.lib.mcle_pinv(self.ctx, d_A.ptr, m, n, float(rcond), out.ptr, b))
        out = out.get()
        return out[0] if single else out

    def run_bd(self, K, nr, n_symbols, iPu, noise_var, seed, first, count, bd_noise_var=1e-50, pathloss=None,
               waterfilling=True, method=DEMOD_MINDIST, dtype=None, per_realization=False, counters=None):
        """apps/comp_BD/simulate_comp_simple.py:95-140 fused (no external interference): K cells of nr x nr
        antennas, joint block-diagonalising precoder, zero forcing at the users; n_symbols per stream."""
        cfg = _lib.BdCfg()
        cfg.K, cfg.nr, cfg.n_symbols, cfg.demod_method = int(K), int(nr), int(n_symbols), int(method)
        cfg.waterfilling, cfg.has_pathloss = (1 if waterfilling else 0), (0 if pathloss is None else 1)
        cfg.iPu, cfg.noise_var, cfg.bd_noise_var = float(iPu), float(noise_var), float(bd_noise_var)
        if pathloss is not None:
            pl = np.asarray(pathloss, dtype=np.float64)
            if pl.shape != (K, K) or K > 4:
                raise ValueError("pathloss must be a [K, K] matrix (rx user, tx user), K <= 4")
            for i, v in enumerate(pl.reshape(-1)):
                cfg.pathloss[i] = float(v)
        return self._run(self.lib.mcle_run_bd, cfg, seed, first, count, dtype, per_realization, counters)

    def run_comp(self, K, r, n_ext, n_symbols, iPu, noise_var, pe, seed, first, count, variant="None", num_streams=1,
                 packet_length=60, pathloss=None, pathloss_ext=None, pathloss_per_realization=None, sinr_pe=1.0,
                 method=DEMOD_MINDIST, dtype=None, per_realization=False, counters=None):
        """apps/comp_BD/simulate_comp.py fused (csrc/pipeline_comp.hip, include/mcle.h at mcle_run_comp): K cells of r x r
        antennas, n_ext interferer antennas of power pe, one of the app's variants 'None' / 'naive' / 'fixed' / 'capacity' /
        'effec_throughput' / 'Whitening'; n_symbols per kept stream.  pathloss [K, K] (rx user, tx user) and pathloss_ext
        [K, n_ext], or pathloss_per_realization [count, K, K + n_ext] (host or device array).
        -> the counters dict; with per_realization=True (counters, dict(sym_err [count], bit_err [count],
        stream_sym_err [count, K r], stream_bit_err [count, K r], ns [count, K], sinr [count, K r]))."""
        if variant not in _lib.COMP_VARIANTS:
            raise ValueError("unknown variant %r (known: None, naive, fixed, capacity, effec_throughput, Whitening)" % (variant,))
        K, r, n_ext, count = int(K), int(r), int(n_ext), int(count)
        cfg = _lib.CompCfg()
        cfg.K, cfg.r, cfg.n_ext, cfg.n_symbols, cfg.demod_method = K, r, n_ext, int(n_symbols), int(method)
        cfg.method, cfg.metric = _lib.COMP_VARIANTS[variant]
        cfg.num_streams, cfg.packet_length = int(num_streams), int(packet_length)
        cfg.iPu, cfg.noise_var, cfg.pe, cfg.sinr_pe = float(iPu), float(noise_var), float(pe), float(sinr_pe)
        in_envelope = 1 <= K <= 4 and 0 <= n_ext <= 8           # anything else is refused by the library below
        if (pathloss is None) != (pathloss_ext is None) and n_ext > 0:
            raise ValueError("pathloss and pathloss_ext go together")
        if pathloss is not None and in_envelope:
            pl = np.asarray(pathloss, dtype=np.float64)
            ple = np.zeros((K, 0)) if pathloss_ext is None else np.asarray(pathloss_ext, dtype=np.float64)
            if pl.shape != (K, K) or ple.shape != (K, n_ext):
                raise ValueError("pathloss must be [K, K] (rx user, tx user) and pathloss_ext [K, n_ext]")
            cfg.has_pathloss = 1
            for i, v in enumerate(pl.reshape(-1)):
                cfg.pathloss[i] = float(v)
            for i, v in enumerate(ple.reshape(-1)):
                cfg.pathloss_ext[i] = float(v)
        d_pl = None
        if pathloss_per_realization is not None and in_envelope:
            d_pl = pathloss_per_realization
            if not isinstance(d_pl, DeviceArray):
                d_pl = self.to_device(np.ascontiguousarray(d_pl, dtype=np.float64))
            if tuple(d_pl.shape) != (count, K, K + n_ext) or d_pl.dtype != np.dtype(np.float64):
                raise ValueError("pathloss_per_realization must be float64 [count, K, K + n_ext]")
        dt = self._dt(dtype)
        cnt = counters if counters is not None else self.zeros(1, np.dtype((np.void, ctypes.sizeof(Counters))))
        out = {}
        if per_realization:
            n = K * r if in_envelope and 1 <= r <= 4 else 0
            out = dict(sym_err=self.empty(count, np.uint32), bit_err=self.empty(count, np.uint32),
                       stream_sym_err=self.empty((count, n), np.uint32), stream_bit_err=self.empty((count, n), np.uint32),
                       ns=self.empty((count, K), np.int32), sinr=self.empty((count, n), np.float64))
        ptr = lambda name: out[name].ptr if per_realization else None
        self._raise_value(self.lib.mcle_run_comp(self.ctx, dt, byref(cfg), int(seed), int(first), count,
                                                 d_pl.ptr if (d_pl is not None and count) else None, cnt.ptr, ptr("sym_err"),
                                                 ptr("bit_err"), ptr("stream_sym_err"), ptr("stream_bit_err"), ptr("ns"),
                                                 ptr("sinr")))
        if counters is not None and not per_realization:
            return None
        res = None if counters is not None else self._counters(cnt)
        if per_realization:
            return res, {k: v.get() for k, v in out.items()}
        return res

    # ---- pilot-based channel estimation (csrc/kernels_chanest.hip) ------------------------------------
    def cazac_estimate(self, ref_seq, rx, num_taps_to_keep, size_multiplier=2, normalized=False, cover=None, dtype=None):
        """CazacBasedChannelEstimator.estimate_channel_freq_domain on rows: ref_seq [ne]; rx [..., ne], or
        [..., n_cover, ne] with a (real) cover code, whose axis is averaged out first -> [..., size_multiplier * ne]."""
        dt = self._dt(dtype)
        d_ref, _ = self._cin(ref_seq, dt)
        d_rx, host = self._cin(rx, dt)
        ne = d_ref.size
        n_cover, c_ptr = 1, None
        if cover is not None:
            cov = np.ascontiguousarray(cover, dtype=np.float64).reshape(-1)
            n_cover, c_ptr = cov.size, cov.ctypes.data_as(ctypes.POINTER(c_double))
        lead = d_rx.shape[:-1] if cover is None else d_rx.shape[:-2]
        if d_rx.shape[-1] != ne or (cover is not None and (len(d_rx.shape) < 2 or d_rx.shape[-2] != n_cover)):
            raise ValueError("rx must be [..., %sne = %d] (got %s)" % ("n_cover = %d, " % n_cover if cover is not None else "",
                                                                      ne, d_rx.shape))
        rows = int(np.prod(lead)) if lead else 1
        out = self.empty(tuple(lead) + (int(size_multiplier) * ne,), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_cazac_estimate(self.ctx, dt, d_ref.ptr, ne, d_rx.ptr, rows, n_cover, c_ptr,
                                                       int(num_taps_to_keep), int(size_multiplier),
                                                       1 if normalized else 0, out.ptr))
        return self._out(out, host)

    def run_chanest(self, ref_seqs, n_rx, num_taps_to_keep, size_multiplier, noise_var, tap_power, tap_delay, seed, first,
                    count, normalized=False, dtype=None, per_realization=False):
        """Fused estimation-error Monte Carlo (mcle_run_chanest): ref_seqs [n_users, ne] are the users' sequences on one
        comb, every (user, antenna) link a block-static tapped delay line.  Returns dict(n_realizations, err, pow): per
        user the sums over the realizations, in index order on the host, of sum_{a,k} |H^ - H|^2 and sum_{a,k} |H|^2;
        with per_realization=True also the two [count, n_users] arrays."""
        dt = self._dt(dtype)
        seqs = np.atleast_2d(np.asarray(ref_seqs))
        d_seq = self.to_device(seqs, _lib.np_complex(dt))
        cfg = _lib.ChanestCfg()
        cfg.ne, cfg.size_multiplier, cfg.num_taps_to_keep = int(seqs.shape[1]), int(size_multiplier), int(num_taps_to_keep)
        cfg.n_users, cfg.n_rx, cfg.n_taps, cfg.normalized = int(seqs.shape[0]), int(n_rx), len(tap_delay), 1 if normalized else 0
        cfg.noise_var = float(noise_var)
        if len(tap_delay) > _lib.MAX_TAPS or len(tap_power) != len(tap_delay):
            raise ValueError("at most %d taps; powers and delays must match" % _lib.MAX_TAPS)
        for i, (p, d) in enumerate(zip(tap_power, tap_delay)):
            cfg.tap_power[i], cfg.tap_delay[i] = float(p), int(d)
        cfg.d_ref_seq = d_seq.ptr
        err, pw = self.empty((count, seqs.shape[0]), np.float64), self.empty((count, seqs.shape[0]), np.float64)
        self._raise_value(self.lib.mcle_run_chanest(self.ctx, dt, byref(cfg), int(seed), int(first), int(count), err.ptr,
                                                    pw.ptr))
        e, p = err.get(), pw.get()
        # (cumsum adds strictly in index order; a plain sum may go pairwise)
        tot = [np.cumsum(v, axis=0)[-1] if count else np.zeros(seqs.shape[0]) for v in (e, p)]
        res = {"n_realizations": int(count), "err": tot[0], "pow": tot[1]}
        return (res, e, p) if per_realization else res

    # ---- interference cancellation (csrc/kernels_chanest_ic.hip) --------------------------------------
    def cazac_cancel(self, ref_seq, rx, est, size_multiplier=2, dtype=None, out=None):
        """rx - est[..., ::size_multiplier] * ref_seq: the contribution of an estimated user taken out of the comb.  ref_seq
        [ne]; rx [..., ne]; est [..., size_multiplier * ne] as cazac_estimate returns it.  out: a DeviceArray shaped like rx
        to write into (rx itself: in place), which is then also what is returned."""
        dt = self._dt(dtype)
        d_ref, _ = self._cin(ref_seq, dt)
        d_rx, host = self._cin(rx, dt)
        d_est, _ = self._cin(est, dt)
        ne, m = d_ref.size, int(size_multiplier)
        if d_rx.shape[-1] != ne or tuple(d_est.shape) != tuple(d_rx.shape[:-1]) + (m * ne,):
            raise ValueError("rx must be [..., ne = %d] and est [..., %d] over the same rows (got %s, %s)"
                             % (ne, m * ne, d_rx.shape, d_est.shape))
        if out is None:
            out = self.empty(d_rx.shape, _lib.np_complex(dt))
        elif not isinstance(out, DeviceArray) or out.dtype != d_rx.dtype or tuple(out.shape) != tuple(d_rx.shape):
            raise ValueError("out must be a device array with rx's shape and type")
        else:
            host = False
        self._raise_value(self.lib.mcle_cazac_cancel(self.ctx, dt, d_ref.ptr, ne, d_rx.ptr, d_est.ptr, d_rx.size // max(ne, 1), m,
                                                     out.ptr))
        return self._out(out, host)

    def run_chanest_ic(self, ref_seqs, n_rx, num_taps_to_keep, size_multiplier, noise_var, tap_power, tap_delay, seed, first,
                       count, mode, direct_user=0, link_gain=None, normalized=False, dtype=None, per_realization=False,
                       return_order=False):
        """run_chanest with a linear power gain per user (link_gain, default all 1) and interference cancellation at the
        receiver of `direct_user` (mcle_run_chanest_ic).  mode 0 / 'none': every user from the received comb; 1 / 'direct':
        the direct user is estimated and subtracted first; 2 / 'sic': then the others in descending order of the norm of their
        first estimates, each estimated from the residual left by all stronger ones.  Returns what run_chanest returns; with
        return_order=True the int32 array [count, n_users] of the order of the final estimates is appended."""
        dt = self._dt(dtype)
        seqs = np.atleast_2d(np.asarray(ref_seqs))
        n_users = int(seqs.shape[0])
        d_seq = self.to_device(seqs, _lib.np_complex(dt))
        ic = _lib.ChanestIcCfg()
        cfg = ic.base
        cfg.ne, cfg.size_multiplier, cfg.num_taps_to_keep = int(seqs.shape[1]), int(size_multiplier), int(num_taps_to_keep)
        cfg.n_users, cfg.n_rx, cfg.n_taps, cfg.normalized = n_users, int(n_rx), len(tap_delay), 1 if normalized else 0
        cfg.noise_var = float(noise_var)
        if len(tap_delay) > _lib.MAX_TAPS or len(tap_power) != len(tap_delay):
            raise ValueError("at most %d taps; powers and delays must match" % _lib.MAX_TAPS)
        for i, (p, d) in enumerate(zip(tap_power, tap_delay)):
            cfg.tap_power[i], cfg.tap_delay[i] = float(p), int(d)
        cfg.d_ref_seq = d_seq.ptr
        ic.mode, ic.direct_user = int(_lib.CHANEST_IC_MODES.get(mode, mode)), int(direct_user)
        gains = np.ones(n_users) if link_gain is None else np.asarray(link_gain, dtype=np.float64).reshape(-1)
        if gains.size != n_users:
            raise ValueError("link_gain must hold one gain per user (%d users, got %d)" % (n_users, gains.size))
        for u in range(min(n_users, 8)):
            ic.link_gain[u] = float(gains[u])
        err, pw = self.empty((count, n_users), np.float64), self.empty((count, n_users), np.float64)
        order = self.empty((count, n_users), np.int32) if return_order else None
        self._raise_value(self.lib.mcle_run_chanest_ic(self.ctx, dt, byref(ic), int(seed), int(first), int(count), err.ptr,
                                                       pw.ptr, order.ptr if return_order else None))
        e, p = err.get(), pw.get()
        # (cumsum adds strictly in index order; a plain sum may go pairwise)
        tot = [np.cumsum(v, axis=0)[-1] if count else np.zeros(n_users) for v in (e, p)]
        res = {"n_realizations": int(count), "err": tot[0], "pow": tot[1]}
        ret = (res, e, p) if per_realization else (res,)
        if return_order:
            ret = ret + (order.get(),)
        return ret if len(ret) > 1 else res

    # ---- LS / MMSE block-pilot estimators (csrc/kernels_estimators.hip) --------------------------------
    @staticmethod
    def _host_c128(M, nr, name):
        """[nr, nr] complex matrix -> (contiguous complex128 array, POINTER(c_double) to its interleaved re, im)"""
        M = np.ascontiguousarray(M, dtype=np.complex128)
        if M.shape != (nr, nr):
            raise ValueError("%s must be [%d, %d] (got %s)" % (name, nr, nr, M.shape))
        return M, M.view(np.float64).ctypes.data_as(ctypes.POINTER(c_double))

    def _pilot_args(self, Y, s, dt, nt_fixed=None):
        """Y [batch, nr, P] and s [nt, P] or [batch, nt, P] -> device arrays, shapes and whether s is per realization"""
        d_Y, host = self._cin(Y, dt)
        d_s, _ = self._cin(s, dt)
        if len(d_Y.shape) != 3 or len(d_s.shape) not in (2, 3):
            raise ValueError("Y must be [batch, nr, n_pilots] and s [nt, n_pilots] or [batch, nt, n_pilots] (got %s, %s)"
                             % (d_Y.shape, d_s.shape))
        batch, nr, P = (int(v) for v in d_Y.shape)
        per = len(d_s.shape) == 3
        nt = int(d_s.shape[-2])
        if int(d_s.shape[-1]) != P or (per and int(d_s.shape[0]) != batch):
            raise ValueError("s %s does not match Y %s" % (d_s.shape, d_Y.shape))
        if nt_fixed is not None and nt != nt_fixed:
            raise ValueError("the MMSE estimator needs nt = %d (got %d)" % (nt_fixed, nt))
        return d_Y, d_s, host, batch, nr, nt, P, per

    def ls_estimate(self, Y, s, dtype=None):
        """compute_ls_estimation on a batch: Y [batch, nr, P]; s [nt, P] (shared) or [batch, nt, P] -> Y s^H (s s^H)^-1,
        [batch, nr, nt].  One launch (mcle_ls_estimate)."""
        dt = self._dt(dtype)
        d_Y, d_s, host, batch, nr, nt, P, per = self._pilot_args(Y, s, dt)
        out = self.empty((batch, nr, nt), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_ls_estimate(self.ctx, dt, d_Y.ptr, d_s.ptr, nr, nt, P, 1 if per else 0, batch, out.ptr))
        return self._out(out, host)

    def mmse_estimate(self, Y, s, noise_power, C, dtype=None):
        """compute_mmse_estimation on a batch: Y [batch, nr, P]; s [1, P] or [batch, 1, P]; C [nr, nr] (host) ->
        (noise_power I + P C)^-1 C (Y s^H) P / |s|^2, [batch, nr, 1].  One launch (mcle_mmse_estimate)."""
        dt = self._dt(dtype)
        d_Y, d_s, host, batch, nr, nt, P, per = self._pilot_args(Y, s, dt, nt_fixed=1)
        C, c_ptr = self._host_c128(C, nr, "C")
        out = self.empty((batch, nr, 1), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_mmse_estimate(self.ctx, dt, d_Y.ptr, d_s.ptr, nr, P, 1 if per else 0, batch,
                                                      float(noise_power), c_ptr, out.ptr))
        return self._out(out, host)

    def run_pilot_mse(self, nr, nt, n_pilots, noise_power, seed, first, count, pilot_power=1.0, alpha=1.0, pilots=None,
                      chan_factor=None, cov=None, dtype=None, per_realization=False):
        """Fused estimation-error Monte Carlo of the LS and MMSE estimators (mcle_run_pilot_mse): per realization pilots
        (drawn with power pilot_power, or `pilots` [nt, n_pilots]), h = alpha chan_factor w, Y = h s + noise, both
        estimates from the same Y; the MMSE one only with `cov` (the C handed to it; needs nt = 1).  Returns
        dict(n_realizations, err_ls, err_mmse, pow): the sums over the realizations, in index order on the host, of
        |h^ - h|_F^2 and |h|_F^2 (err_mmse None without cov); with per_realization=True also the three [count] arrays."""
        dt = self._dt(dtype)
        cfg = _lib.PilotMseCfg()
        cfg.nr, cfg.nt, cfg.n_pilots = int(nr), int(nt), int(n_pilots)
        cfg.pilot_power, cfg.noise_power, cfg.alpha = float(pilot_power), float(noise_power), float(alpha)
        cfg.random_pilots = 1 if pilots is None else 0
        keep = []
        if pilots is not None:
            d_p = self.to_device(np.asarray(pilots).reshape(int(nt), int(n_pilots)), _lib.np_complex(dt))
            keep.append(d_p)
            cfg.d_pilots = d_p.ptr
        if chan_factor is not None:
            L, cfg.chan_factor = self._host_c128(chan_factor, int(nr), "chan_factor")
            keep.append(L)
        if cov is not None:
            Cm, cfg.cov = self._host_c128(cov, int(nr), "cov")
            keep.append(Cm)
        e_ls, pw = self.empty(count, np.float64), self.empty(count, np.float64)
        e_mm = self.empty(count, np.float64) if cov is not None else None
        self._raise_value(self.lib.mcle_run_pilot_mse(self.ctx, dt, byref(cfg), int(seed), int(first), int(count), e_ls.ptr,
                                                      e_mm.ptr if e_mm is not None else None, pw.ptr))
        arrs = [a.get() if a is not None else None for a in (e_ls, e_mm, pw)]
        # (cumsum adds strictly in index order; a plain sum may go pairwise)
        tot = [None if a is None else (float(np.cumsum(a)[-1]) if count else 0.0) for a in arrs]
        res = {"n_realizations": int(count), "err_ls": tot[0], "err_mmse": tot[1], "pow": tot[2]}
        return (res, arrs[0], arrs[1], arrs[2]) if per_realization else res

    def run_mimo_pilot_link(self, nt, nr, n_pilots, n_symbols, noise_var, seed, first, count, pilot_power=1.0, alpha=1.0,
                            pilots=None, chan_factor=None, cov=None, estimator="ls", mmse=False, method=DEMOD_MINDIST,
                            dtype=None, per_realization=False):
        """The flat Blast link with pilot-estimated and with perfect channel state on the same draws
        (mcle_run_mimo_pilot_link): per realization H = alpha chan_factor W, a block of n_pilots pilots (drawn with power
        pilot_power, or `pilots` [nt, n_pilots]), the LS estimate -- or with estimator='mmse' (nt = 1) the MMSE one for the
        covariance `cov` [nr, nr], turned here into B = (noise_var I + n_pilots cov)^-1 cov --, the Blast filter from the
        estimate and from H (mmse=True: set_noise_var(noise_var)), n_symbols per layer.  Returns (counters with estimated
        CSI, counters with perfect CSI); with per_realization=True also sym_err [2, count], bit_err [2, count] (row 0
        estimated, row 1 perfect; 0xFFFFFFFF marks a skipped realization), err [count] = |H^ - H|_F^2, pow [count] = |H|_F^2."""
        return self._pilot_link(self.lib.mcle_run_mimo_pilot_link, nt, nr, n_pilots, n_symbols, noise_var, seed, first, count,
                                pilot_power, alpha, pilots, chan_factor, cov, estimator, mmse, method, dtype, per_realization)

    def run_mimo_large_pilot_link(self, nt, nr, n_pilots, n_symbols, noise_var, seed, first, count, pilot_power=1.0, alpha=1.0,
                                  pilots=None, chan_factor=None, cov=None, estimator="ls", mmse=False, method=DEMOD_MINDIST,
                                  dtype=None, per_realization=False):
        """run_mimo_pilot_link for large arrays (mcle_run_mimo_large_pilot): 1 <= nt <= 8, nt <= nr <= 16, the walk of
        run_mimo_large on the matrix cores through the filter of the estimate and that of the channel at once.  Same
        arguments, same return value, same draws: up to 4 x 4 the realizations of run_mimo_pilot_link, and with no chan_factor
        and alpha = 1 the perfect-CSI block is run_mimo_large on the same (seed, first, count)."""
        return self._pilot_link(self.lib.mcle_run_mimo_large_pilot, nt, nr, n_pilots, n_symbols, noise_var, seed, first, count,
                                pilot_power, alpha, pilots, chan_factor, cov, estimator, mmse, method, dtype, per_realization)

    def _pilot_link(self, entry, nt, nr, n_pilots, n_symbols, noise_var, seed, first, count, pilot_power, alpha, pilots,
                    chan_factor, cov, estimator, mmse, method, dtype, per_realization):
        """The call both pilot links share: `entry` is the library's entry point."""
        dt = self._dt(dtype)
        nt, nr, P, count = int(nt), int(nr), int(n_pilots), int(count)
        if estimator not in _lib.PILOT_ESTIMATORS:
            raise ValueError("estimator must be 'ls' or 'mmse' (got %r)" % (estimator,))
        cfg = _lib.MimoPilotCfg(nt, nr, P, int(n_symbols), int(method), _lib.PILOT_ESTIMATORS[estimator],
                                1 if pilots is None else 0, 1 if mmse else 0, float(noise_var), float(pilot_power),
                                float(alpha))
        d_p = d_L = d_B = None
        if pilots is not None:
            s = np.asarray(pilots, dtype=np.complex128)
            if s.shape != (nt, P):
                raise ValueError("pilots must be [nt, n_pilots] = [%d, %d] (got %s)" % (nt, P, s.shape))
            d_p = self.to_device(s, np.complex128)
        if chan_factor is not None:
            d_L = self.to_device(self._host_c128(chan_factor, nr, "chan_factor")[0], np.complex128)
        if estimator == "mmse" and cov is not None:          # (nt > 1 or no covariance: the library refuses)
            C = self._host_c128(cov, nr, "cov")[0]
            M = float(noise_var) * np.eye(nr) + P * C
            if not (np.all(np.isfinite(M)) and np.linalg.matrix_rank(M) == nr):
                raise ValueError("noise_var * I + n_pilots * cov is singular")
            d_B = self.to_device(np.linalg.solve(M, C), np.complex128)
        cnt = self.zeros(2, np.dtype((np.void, ctypes.sizeof(Counters))))
        se = be = err = pw = None
        if per_realization:
            se, be = self.empty((2, count), np.uint32), self.empty((2, count), np.uint32)
            err, pw = self.empty(count, np.float64), self.empty(count, np.float64)
        self._raise_value(entry(
            self.ctx, dt, byref(cfg), int(seed), int(first), count, d_p.ptr if d_p is not None else None,
            d_L.ptr if d_L is not None else None, d_B.ptr if d_B is not None else None, cnt.ptr,
            se.ptr if per_realization else None, be.ptr if per_realization else None,
            err.ptr if per_realization else None, pw.ptr if per_realization else None))
        raw = cnt.get().tobytes()
        size = ctypes.sizeof(Counters)
        res = tuple(Counters.from_buffer_copy(raw[i * size:(i + 1) * size]).as_dict() for i in range(2))
        if per_realization:
            return res + (se.get(), be.get(), err.get(), pw.get())
        return res

    # ---- Grassmannian codebooks (csrc/kernels_codebook.hip) -------------------------------------------
    def chordal_min_dist(self, codebooks, dtype=None, full=False):
        """Squared chordal distances of codebooks [n, K, Nt, Ns] (or one [K, Nt, Ns]) (mcle_chordal_min_dist): returns
        (min_d2 [n] float64, pair [n, 2] int32), with full=True also the symmetric d^2 matrices [n, K, K]; the leading axis
        is dropped for a single codebook."""
        dt = self._dt(dtype)
        d_cb, _ = self._cin(codebooks, dt)
        single = len(d_cb.shape) == 3
        if len(d_cb.shape) not in (3, 4):
            raise ValueError("codebooks must be [n, K, Nt, Ns] or [K, Nt, Ns] (got %s)" % (d_cb.shape,))
        n = 1 if single else int(d_cb.shape[0])
        K, Nt, Ns = (int(v) for v in d_cb.shape[-3:])
        md2, pair = self.empty(n, np.float64), self.empty((n, 2), np.int32)
        d2 = self.empty((n, K, K), np.float64) if full else None
        self._raise_value(self.lib.mcle_chordal_min_dist(self.ctx, dt, d_cb.ptr, n, K, Nt, Ns, md2.ptr, pair.ptr,
                                                         d2.ptr if full else None))
        out = [md2.get(), pair.get()] + ([d2.get()] if full else [])
        return tuple(v[0] for v in out) if single else tuple(out)

    def codebook_generate(self, K, Nt, Ns, seed, first, count, codebook_type="complex", dtype=None, device=False):
        """The search's candidates [first, first + count) of `seed` as they are before orthonormalisation
        (mcle_codebook_generate): [count, K, Nt, Ns] complex."""
        dt = self._dt(dtype)
        out = self.empty((count, K, Nt, Ns), _lib.np_complex(dt))
        self._raise_value(self.lib.mcle_codebook_generate(self.ctx, dt, int(_lib.CODEBOOK_TYPES.get(codebook_type, codebook_type)),
                                                          int(K), int(Nt), int(Ns), int(seed), int(first), int(count), out.ptr))
        return out if device else out.get()

    def run_codebook_search(self, K, Nt, Ns, seed, first, count, codebook_type="complex", dtype=None, per_candidate=False):
        """Fused random codebook search over the candidates [first, first + count) (mcle_run_codebook_search).  Returns
        dict(best_index, best_min_d2, pair, n_candidates); with per_candidate=True also min_d2 [count] and pair [count, 2]."""
        dt = self._dt(dtype)
        cfg = _lib.CodebookCfg(int(K), int(Nt), int(Ns), int(_lib.CODEBOOK_TYPES.get(codebook_type, codebook_type)))
        res = _lib.CodebookResult()
        md2 = self.empty(count, np.float64) if per_candidate else None
        pair = self.empty((count, 2), np.int32) if per_candidate else None
        self._raise_value(self.lib.mcle_run_codebook_search(self.ctx, dt, byref(cfg), int(seed), int(first), int(count), byref(res),
                                                            md2.ptr if per_candidate else None,
                                                            pair.ptr if per_candidate else None))
        out = {"best_index": int(res.best_index), "best_min_d2": float(res.best_min_d2),
               "pair": (int(res.pair[0]), int(res.pair[1])), "n_candidates": int(res.n_candidates)}
        return (out, md2.get(), pair.get()) if per_candidate else out

    # ---- same-seed parity mode (NumPy legacy RandomState on the device) ----------------------
    def legacy_draws(self, program, seed_base, first, count):
        """program: list of ('randint', n, range) / ('randn', n) / ('rand', n).  Realization r gets
        what NumPy draws after np.random.seed(seed_base + first + r).  Returns (ints DeviceArray
        [count, n_int] int32, doubles DeviceArray [count, n_dbl] float64)."""
        kinds = {"randint": 0, "randn": 1, "rand": 2}
        segs = (LegacySeg * len(program))()
        n_int = n_dbl = 0
        for i, item in enumerate(program):
            k = kinds[item[0]]
            segs[i].kind, segs[i].n = k, int(item[1])
            segs[i].range = int(item[2]) if k == 0 else 0
            if k == 0:
                n_int += int(item[1])
            else:
                n_dbl += int(item[1])
        ints = self.empty((count, max(n_int, 1)), np.int32)
        dbls = self.empty((count, max(n_dbl, 1)), np.float64)
        status = self.zeros(count, np.uint32)
        check(self.lib.mcle_legacy_draws(self.ctx, segs, len(program), int(seed_base) & 0xFFFFFFFF, int(first),
                                         int(count), ints.ptr, max(n_int, 1), dbls.ptr, max(n_dbl, 1), status.ptr))
        if status.get().any():
            raise McleError("legacy draw program ran out of words")
        return ints, dbls

    def complex_from_parts(self, re, im, scale=1.0, dtype=None):
        """scale * (re + 1j*im) on the device from two float64 arrays (host or device)."""
        dt = self._dt(dtype)
        d_re = re if isinstance(re, DeviceArray) else self.to_device(np.asarray(re), np.float64)
        d_im = im if isinstance(im, DeviceArray) else self.to_device(np.asarray(im), np.float64)
        out = self.empty(d_re.shape, _lib.np_complex(dt))
        check(self.lib.mcle_complex_from_parts(self.ctx, dt, d_re.ptr, d_im.ptr, float(scale), out.ptr, d_re.size))
        return out


_default = {}


def default_device():
    """Device of this process: torch's current device once torch.distributed is initialised (the launcher set it
    per rank), else LOCAL_RANK of the launcher's environment, else 0 -- so that the mirror classes and simulators
    of every rank compute on that rank's GPU instead of all piling onto GPU 0."""
    import os
    import sys
    torch = sys.modules.get("torch")          # only if the process uses torch already: importing it here would cost every
    if torch is not None:                     # torch-free caller seconds and bind torch's bundled HIP / RCCL libraries
        dist = getattr(torch, "distributed", None)
        try:
            if dist is not None and dist.is_available() and dist.is_initialized() and torch.cuda.is_available():
                return int(torch.cuda.current_device())
        except Exception:
            pass
    for key in ("LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "SLURM_LOCALID"):
        if key in os.environ:
            try:
                n = _lib.device_count()
            except McleError:
                n = 0
            return int(os.environ[key]) % n if n > 0 else 0
    return 0


def get_engine(device=None):
    """Process-wide default engine per device (created on first use); device None = default_device()."""
    if device is None:
        device = default_device()
    eng = _default.get(device)
    if eng is None:
        eng = _default[device] = Engine(device)
    return eng
