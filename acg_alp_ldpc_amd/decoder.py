"""Host-side mirror of the reference's Decoder operator API (algo/algo.h:6-11).

    BeliefPropagationDecoder(max_iter)                     algo/bp.h:208-222
    QPADMMDecoder(alpha, mu, max_iter=2000, eps_stop=1e-5) algo/qp_admm.h:180-194
    MinSumDecoder(max_iter, scale)                         build-added, not in the reference
    QuantizedMinSumDecoder(max_iter, quant)                build-added, not in the reference: fixed-point layered min-sum
    StreamedQuantizedMinSumDecoder(max_iter, quant)        build-added: the same decoder, state in device memory, any code
    StreamedLayeredBPDecoder(max_iter)                     build-added: layered sum-product, state in device memory, any code
    StreamedLayeredMinSumDecoder(max_iter, scale)          build-added: layered min-sum, state in device memory, any code
    OSDDecoder(order=1)                                    build-added, not in the reference: ordered-statistics decoding

    decode(H, channel_word, snr) -> (codeword, ok)         same argument meaning as algo/algo.h:8:
        H: m x n 0/1 matrix (or a ParityCheckMatrix), channel_word: n raw channel symbols y
        (NOT LLRs), snr: Es/N0 in dB.  BP failure returns (empty array, False) like bp.h:198.
    decode_batch(H, Y, snr) -> (bits[F,n], ok[F], iters[F])
    name() -> "BP" / "QP-ADMM" / "MS" / "QMS" / "OSD"

Every call runs on the GPU through libacg_ldpc_hip.so; there is no CPU path.
"""
import collections
import contextlib
import ctypes as C
import dataclasses
import threading

import numpy as np

from . import _lib
from ._lib import Params, check, lib
from .code import ParityCheckMatrix


class _HandleCache:
    """The analysed-graph cache of a decoder object: device handles keyed on H, least recently used first, a handle in use
    never evicted.  A subclass says where its handles come from (_create) and how they go (_destroy)."""

    # The reference hands H to every decode() (algo/algo.h:8) and its optimize_H loop hands a NEW H per proposal to one
    # shared decoder (optimize_H.cpp:16-25,89-104): the analysed-graph cache is therefore bounded.  Least recently used
    # handles beyond MAX_HANDLES are destroyed (device memory, streams and events go with them).
    MAX_HANDLES = 8

    def __init__(self, max_handles=None):
        self.max_handles = int(max_handles) if max_handles else self.MAX_HANDLES
        self._handles = collections.OrderedDict()  # analysed-graph cache keyed on H (SURVEY §8b "Inputs"), LRU order
        self._pins = collections.Counter()         # calls in flight per key: a handle in use is never evicted
        self._lock = threading.RLock()             # (ctypes calls release the GIL: one decoder object may be used from threads)

    def _create(self, code, p, h):
        """the create call of the C ABI this class's handles come from (p: what _params() returned) -> its return code"""
        raise NotImplementedError

    def _destroy(self, h):
        """the destroy call for a handle of _create"""
        raise NotImplementedError

    def _params(self):
        raise NotImplementedError

    def _key(self, H):
        """ParityCheckMatrix objects are keyed on identity (they are immutable); dense arrays on their CONTENT: shape + the
        packed bits themselves (5.6 KB for 160 x 280), compared for equality by the dict — a hash alone could collide and
        silently decode against the wrong graph."""
        if isinstance(H, ParityCheckMatrix):
            return ("pcm", id(H))
        a = np.ascontiguousarray(H)
        if a.ndim != 2:
            raise ValueError("H must be an m x n matrix")
        return ("dense", a.shape, np.packbits(a != 0).tobytes())

    def handle(self, H):
        """(device handle, ParityCheckMatrix) for H — valid until max_handles OTHER matrices have been used through this object;
        the decode calls below pin theirs for the duration of the call."""
        with self._lock:
            return self._lookup(self._key(H), H)

    def _lookup(self, k, H):
        ent = self._handles.get(k)
        if ent is not None:
            self._handles.move_to_end(k)
            return ent
        code = H if isinstance(H, ParityCheckMatrix) else ParityCheckMatrix(H)
        h = C.c_void_p()
        p = self._params()
        check(self._create(code, p, h))
        ent = (h, code)
        self._handles[k] = ent
        self._trim()
        return ent

    def _trim(self):
        if len(self._handles) <= self.max_handles:
            return
        for k in list(self._handles):           # least recently used first; never the newest, never one in use
            if len(self._handles) <= self.max_handles:
                break
            if self._pins[k] == 0 and k != next(reversed(self._handles)):
                old, _ = self._handles.pop(k)
                self._destroy(old)   # synchronises the handle's stream first

    @contextlib.contextmanager
    def _lease(self, H):
        """the handle for H, kept out of the eviction's reach while a call uses it"""
        with self._lock:
            k = self._key(H)
            ent = self._lookup(k, H)
            self._pins[k] += 1
        try:
            yield ent
        finally:
            with self._lock:
                self._pins[k] -= 1
                self._trim()

    def live_handles(self):
        return len(self._handles)

    def close(self):
        with self._lock:
            for h, _ in self._handles.values():
                self._destroy(h)
            self._handles = collections.OrderedDict()
            self._pins.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Decoder(_HandleCache):
    _algo = None
    _name = None   # name() where the algorithm alone does not give it

    def __init__(self, max_iter, early_exit=True, precision=_lib.PREC_DEFAULT, device=-1, lanes_per_frame=0,
                 engine=_lib.ENGINE_AUTO, schedule=_lib.SCHEDULE_FLOODING, fast_setup=False, max_handles=None):
        super().__init__(max_handles)
        self.max_iter = int(max_iter)
        self.early_exit = bool(early_exit)
        self.precision = precision
        self.device = device
        self.lanes_per_frame = lanes_per_frame
        self.engine = engine
        self.schedule = schedule
        self.fast_setup = bool(fast_setup)

    # -- parameters -------------------------------------------------------------------------
    def _params(self):
        p = Params()
        lib().acg_ldpc_params_default(C.byref(p))
        p.algo = self._algo
        p.max_iter = self.max_iter
        p.early_exit = 1 if self.early_exit else 0
        p.precision = self.precision
        p.device = self.device
        p.lanes_per_frame = self.lanes_per_frame
        p.engine = self.engine
        p.schedule = self.schedule
        p.fast_setup = 1 if self.fast_setup else 0
        return p

    def _create(self, code, p, h):
        return lib().acg_ldpc_decoder_create(code._h, C.byref(p), C.byref(h))

    def _destroy(self, h):
        lib().acg_ldpc_decoder_destroy(h)

    # -- reference API ----------------------------------------------------------------------
    def name(self):
        return self._name or {_lib.ALGO_BP: "BP", _lib.ALGO_QPADMM: "QP-ADMM", _lib.ALGO_MINSUM: "MS"}[self._algo]

    def decode(self, H, channel_word, snr):
        bits, ok, _ = self.decode_batch(H, np.asarray(channel_word, dtype=np.float64)[None, :], snr)
        if not ok[0] and self._algo != _lib.ALGO_QPADMM:
            return np.zeros(0, dtype=np.uint8), False  # {TCodeword(), false}, bp.h:198
        return bits[0], bool(ok[0])

    def decode_batch(self, H, Y, snr, out=None):
        """Y: frames x n channel symbols.  float64 (default): the reference's exact LLRs; a float32 array travels as
        float32 (half the PCIe bytes, acg_ldpc_decode_batch_f32).  out = (bits, ok, iters) reuses caller arrays."""
        with self._lease(H) as (h, code):
            return self._decode_batch(h, code, Y, snr, out)

    def _decode_batch(self, h, code, Y, snr, out):
        f32 = isinstance(Y, np.ndarray) and Y.dtype == np.float32
        Y = np.ascontiguousarray(Y, dtype=np.float32 if f32 else np.float64)
        if Y.ndim != 2 or Y.shape[1] != code.n:
            raise ValueError("Y must be frames x n")
        F = Y.shape[0]
        if out is not None:
            bits, ok, iters = out
            assert bits.shape == (F, code.n) and bits.dtype == np.uint8 and bits.flags.c_contiguous
            assert ok.shape == (F,) and ok.dtype == np.uint8 and iters.shape == (F,) and iters.dtype == np.int32
        else:
            bits = np.empty((F, code.n), dtype=np.uint8)
            ok = np.empty(F, dtype=np.uint8)
            iters = np.empty(F, dtype=np.int32)
        fn = lib().acg_ldpc_decode_batch_f32 if f32 else lib().acg_ldpc_decode_batch
        check(fn(h, Y.ctypes.data, F, float(snr), bits.ctypes.data, ok.ctypes.data, iters.ctypes.data))
        return bits, ok, iters

    def decode_batch_dev(self, H, y_ptr, y_is_f64, frames, snr, bits_ptr, ok_ptr, iters_ptr=None, stream=None):
        """device pointers (ints); asynchronous on `stream` (None = the decoder's own stream)"""
        with self._lease(H) as (h, _):
            check(lib().acg_ldpc_decode_batch_dev(h, y_ptr, 1 if y_is_f64 else 0, int(frames), float(snr), bits_ptr,
                                                  ok_ptr, iters_ptr, stream))

    def sync(self, H):
        h, _ = self.handle(H)
        check(lib().acg_ldpc_decoder_sync(h))

    def last_kernel_ms(self, H):
        h, _ = self.handle(H)
        return float(lib().acg_ldpc_decoder_last_kernel_ms(h))

    def describe(self, H):
        """one line naming the engine / kernel instance / launch shape of the handle for H"""
        h, _ = self.handle(H)
        buf = C.create_string_buffer(1024)
        lib().acg_ldpc_decoder_describe(h, buf, 1024)
        return buf.value.decode()

    def freeze_stats(self, H, enable=True):
        """(frames frozen, sweeps not run) by the handle's launches since the previous call (acg_ldpc_debug_freeze_stats);
        enable: whether later launches keep counting.  Zeros for a handle without the freeze path."""
        h, _ = self.handle(H)
        a, b = C.c_int64(), C.c_int64()
        check(lib().acg_ldpc_debug_freeze_stats(h, 1 if enable else 0, C.byref(a), C.byref(b)))
        return a.value, b.value

    def freeze_passes(self, H):
        """(store passes, compare passes): the freeze path's detections that only wrote a snapshot / that loaded and compared
        one, counted since the previous call while freeze_stats has counting on (acg_ldpc_debug_freeze_passes)."""
        h, _ = self.handle(H)
        a, b = C.c_int64(), C.c_int64()
        check(lib().acg_ldpc_debug_freeze_passes(h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def streamed_slab(self, H, slab=0):
        """(P [64, n], R [64, E]): the posteriors and messages slab `slab` of the handle for H holds, row l = lane l = frame
        64 tile + l of the tile that used the slab last (acg_ldpc_debug_streamed_slab; the layout and which tile that is: see
        include/acg_ldpc.h).  fp32 and fp32 for the streamed float layered decoders, int16 and int8 for
        StreamedQuantizedMinSumDecoder; edges in processing order.  Any other decoder is refused by the library."""
        h, code = self.handle(H)
        size = C.c_int64()
        check(lib().acg_ldpc_debug_streamed_slab(h, int(slab), None, 0, C.byref(size)))
        tp, tr = (np.int16, np.int8) if isinstance(self, QuantizedMinSumDecoder) else (np.float32, np.float32)
        n, E = code.n, code.E
        nbytes = 64 * (n * np.dtype(tp).itemsize + E * np.dtype(tr).itemsize)
        if nbytes > size.value:
            raise _lib.LdpcError("a slab of %d bytes does not hold P[%d][64] and R[%d][64]" % (size.value, n, E))
        buf = np.empty(nbytes, dtype=np.uint8)
        check(lib().acg_ldpc_debug_streamed_slab(h, int(slab), buf.ctypes.data, nbytes, C.byref(size)))
        split = 64 * n * np.dtype(tp).itemsize
        P = buf[:split].view(tp).reshape(n, 64).T.copy()
        R = buf[split:].view(tr).reshape(E, 64).T.copy()
        return P, R

    def layout(self, H):
        h, _ = self.handle(H)
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        lib().acg_ldpc_decoder_layout(h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return dict(lds_bytes_per_frame=a.value, lanes_per_frame=b.value, frames_per_block=c.value,
                    grid_blocks=d.value)


class BeliefPropagationDecoder(Decoder):
    """algo/bp.h:208-222 — flooding sum-product in the phi domain, early exit at the first zero syndrome."""
    _algo = _lib.ALGO_BP

    def __init__(self, max_iter, **kw):
        super().__init__(max_iter, **kw)


class MinSumDecoder(Decoder):
    """Build-added normalised min-sum (north_star).  Not in the reference: parity unpinned.
    schedule=SCHEDULE_LAYERED: layered (row-block sequential) schedule — about half the sweeps for the same FER.
    With it, lanes_per_frame=256 / 512 / 1024 selects the engine with one workgroup per frame (codes of tens of thousands of
    edges: pass 1024); 0 takes it only where the wavefront-group kernel refuses the code for its size.
    A code with a check of 9 ... 32 variables (high-rate codes) runs on the wide-check workgroup engine whatever
    lanes_per_frame says: 256 / 512 / 1024 as given, 0 = the smallest of them that holds the largest set of checks."""
    _algo = _lib.ALGO_MINSUM

    def __init__(self, max_iter, scale=1.0, **kw):
        super().__init__(max_iter, **kw)
        self.scale = float(scale)

    def _params(self):
        p = super()._params()
        p.ms_scale = self.scale
        return p


class QPADMMDecoder(Decoder):
    """algo/qp_admm.h:180-194 (same defaults: max_iter=2000, eps_stop=1e-5).

    engine=ENGINE_AUTO: the LDS kernels wherever they accept the code, the streamed engine (state in HBM, one lane per
    frame, any code size) where a frame's state does not fit in LDS; ENGINE_STREAMED forces it (lanes_per_frame must be
    0); ENGINE_FUSED never takes it.  See acg_ldpc.h for the streamed engine's workspace."""
    _algo = _lib.ALGO_QPADMM

    def __init__(self, alpha, mu, max_iter=2000, eps_stop=1e-5, **kw):
        super().__init__(max_iter, **kw)
        self.alpha, self.mu, self.eps_stop = float(alpha), float(mu), float(eps_stop)

    def _params(self):
        p = super()._params()
        p.alpha, p.mu, p.eps_stop = self.alpha, self.mu, self.eps_stop
        return p


@dataclasses.dataclass(frozen=True)
class QuantConfig:
    """acg_ldpc_quant (include/acg_ldpc.h): the defaults are acg_ldpc_quant_default's — offset-1 min-sum, 6-bit channel values in
    steps of 0.5 LLR, 6-bit messages, 8-bit posteriors."""
    llr_step: float = 0.5
    ch_bits: int = 6
    msg_bits: int = 6
    post_bits: int = 8
    scale_num: int = 1
    scale_shift: int = 0
    offset: int = 1

    def as_tuple(self):
        return (float(self.llr_step), int(self.ch_bits), int(self.msg_bits), int(self.post_bits), int(self.scale_num),
                int(self.scale_shift), int(self.offset))

    def as_struct(self):
        return _lib.Quant(*self.as_tuple())


class _RmChannel:
    """acg_ldpc_rm_channel_dev on the classes whose engine has a channel-value entrance"""

    def rm_channel_dev(self, H, cfg, pattern, out_ptr, raw_ptr=None, stream=None):
        """cfg: a _lib.McCfg (device noise); pattern: uint8 [n] of _lib.RM_* as experiment.rate_match_pattern returns it, or
        None = all sent.  Device pointers (ints): cfg.frames * n channel values out — float32 LLRs on the streamed layered
        classes, int16 on the quantized ones — as experiment.run_experiment_rm hands them to the decoder, and, where raw_ptr is
        given, cfg.frames int32 raw-error counts; asynchronous on `stream` (None = the decoder's own stream)"""
        with self._lease(H) as (h, code):
            pat = None
            if pattern is not None:
                pat = np.ascontiguousarray(pattern, dtype=np.uint8)
                if pat.shape != (code.n,):
                    raise ValueError("pattern must have n = %d entries" % code.n)
            check(lib().acg_ldpc_rm_channel_dev(h, C.byref(cfg), None if pat is None else pat.ctypes.data, out_ptr, raw_ptr, stream))


class QuantizedMinSumDecoder(_RmChannel, Decoder):
    """Build-added fixed-point layered min-sum (acg_ldpc_decoder_create_quantized; not in the reference): integer channel
    values, messages and posteriors, one workgroup per frame, check degree up to 32.  Bit-true: tests/layered_q_ref.py restates it.
    quant: a QuantConfig, a dict of its fields, or None for the defaults.  The schedule is layered and the algorithm min-sum;
    lanes_per_frame 0, 64, 128, 256, 512 or 1024 = threads of the workgroup.  The library refuses anything else."""
    _algo = _lib.ALGO_MINSUM
    _name = "QMS"

    def __init__(self, max_iter, quant=None, **kw):
        kw.setdefault("schedule", _lib.SCHEDULE_LAYERED)
        super().__init__(max_iter, **kw)
        if quant is None:
            quant = QuantConfig()
        elif isinstance(quant, dict):
            quant = QuantConfig(**quant)
        self.quant = quant

    def _key(self, H):
        return super()._key(H) + ("quant",) + self.quant.as_tuple()

    def _create(self, code, p, h):
        q = self.quant.as_struct()
        return lib().acg_ldpc_decoder_create_quantized(code._h, C.byref(p), C.byref(q), C.byref(h))

    # -- the integer entrance: channel values in, posteriors out (acg_ldpc_decode_batch_q*) ---------
    def quantize(self, H, Y, snr):
        """host symbols (float64, or float32 travelling as float32) -> int16 channel values of the same shape: this decoder's
        quantiser as the symbol entrance applies it (acg_ldpc_debug_quantize).  H is not read: the quantiser knows no code."""
        f32 = isinstance(Y, np.ndarray) and Y.dtype == np.float32
        Y = np.ascontiguousarray(Y, dtype=np.float32 if f32 else np.float64)
        out = np.empty(Y.shape, dtype=np.int16)
        q = self.quant.as_struct()
        check(lib().acg_ldpc_debug_quantize(Y.ctypes.data, 0 if f32 else 1, Y.size, float(snr), C.byref(q), out.ctypes.data))
        return out

    def decode_llr_batch(self, H, C, posteriors=True, out=None):
        """C: frames x n INTEGER channel values (any integer dtype; every value must fit int16; the decoder clamps them to
        +-Cmax).  A punctured position is 0, a shortened one +Cmax (known 0) or -Cmax (known 1).  A floating-point array is
        refused: LLRs are quantised by the caller, or by quantize().
        out = (bits, ok, iters[, post]) reuses caller arrays.  -> (bits[F,n], ok[F], iters[F][, post[F,n] int16])"""
        a = np.asarray(C)
        if a.dtype.kind not in "iu":
            raise TypeError("decode_llr_batch takes integer channel values, not %s: quantise first (quantize())" % a.dtype)
        if a.dtype != np.int16:
            if a.size and (a.min() < -32768 or a.max() > 32767):
                raise ValueError("channel values must fit int16")
            a = a.astype(np.int16)
        a = np.ascontiguousarray(a)
        with self._lease(H) as (h, code):
            if a.ndim != 2 or a.shape[1] != code.n:
                raise ValueError("C must be frames x n")
            F = a.shape[0]
            if out is not None:
                bits, ok, iters = out[:3]
                post = out[3] if posteriors else None
                assert bits.shape == (F, code.n) and bits.dtype == np.uint8 and bits.flags.c_contiguous
                assert ok.shape == (F,) and ok.dtype == np.uint8 and iters.shape == (F,) and iters.dtype == np.int32
                assert post is None or (post.shape == (F, code.n) and post.dtype == np.int16 and post.flags.c_contiguous)
            else:
                bits = np.empty((F, code.n), dtype=np.uint8)
                ok = np.empty(F, dtype=np.uint8)
                iters = np.empty(F, dtype=np.int32)
                post = np.empty((F, code.n), dtype=np.int16) if posteriors else None
            check(lib().acg_ldpc_decode_batch_q(h, a.ctypes.data, F, bits.ctypes.data, ok.ctypes.data, iters.ctypes.data,
                                                post.ctypes.data if post is not None else None))
        return (bits, ok, iters, post) if posteriors else (bits, ok, iters)

    def decode_llr_batch_dev(self, H, c_ptr, frames, bits_ptr, ok_ptr, iters_ptr=None, post_ptr=None, stream=None):
        """device pointers (ints): frames*n int16 channel values in; packed words, flags, iterations and, where post_ptr is
        given, frames*n int16 posteriors out; asynchronous on `stream` (None = the decoder's own stream)"""
        with self._lease(H) as (h, _):
            check(lib().acg_ldpc_decode_batch_q_dev(h, c_ptr, int(frames), bits_ptr, ok_ptr, iters_ptr, post_ptr, stream))

    def quantize_dev(self, H, y_ptr, y_is_f64, count, snr, c_ptr, stream=None):
        """device pointers (ints): `count` symbols -> `count` int16 channel values; asynchronous on `stream`"""
        with self._lease(H) as (h, _):
            check(lib().acg_ldpc_quantize_dev(h, y_ptr, 1 if y_is_f64 else 0, int(count), float(snr), c_ptr, stream))


class StreamedQuantizedMinSumDecoder(QuantizedMinSumDecoder):
    """Build-added (acg_ldpc_decoder_create_quantized_streamed; not in the reference): QuantizedMinSumDecoder with a frame's state in
    device memory instead of LDS — one lane per frame, 2 n + E bytes per frame — for the codes that one refuses: any size, any
    check degree.  Word, flag, iteration and posterior of every frame are equal on every code both accept, and a code whose
    frame fits in LDS is decoded faster there.  Bit-true: tests/streamed_q_ref.py restates it.  The same methods; lanes_per_frame
    must stay 0 and engine ENGINE_AUTO or ENGINE_STREAMED.  CascadeDecoder and run_experiment_quants build and need the LDS engine."""

    def _key(self, H):
        return super()._key(H) + ("streamed",)

    def _create(self, code, p, h):
        q = self.quant.as_struct()
        return lib().acg_ldpc_decoder_create_quantized_streamed(code._h, C.byref(p), C.byref(q), C.byref(h))


class _StreamedLayered(_RmChannel):
    """the create call and handle key of the streamed float layered engine (acg_ldpc_decoder_create_layered_streamed), and its
    LLR entrance: decode_llr_batch / decode_llr_batch_dev, fp32 LLRs in (punctured and shortened positions among them), fp32
    posterior LLRs out.  tests/streamed_layered_io_ref.py restates it."""

    def _key(self, H):
        return super()._key(H) + ("layered-streamed",)

    def _create(self, code, p, h):
        return lib().acg_ldpc_decoder_create_layered_streamed(code._h, C.byref(p), C.byref(h))

    # -- the LLR entrance: LLRs in, posterior LLRs out (acg_ldpc_decode_batch_llr*) -----------------
    def decode_llr_batch(self, H, L, posteriors=True, out=None):
        """L: frames x n LLRs, positive = bit 0 (any real array; converted to float32).  NaN counts as 0 and every value is
        clamped to +-2^20.  A punctured position is 0, a shortened one +2^20 (known 0) or -2^20 (known 1).
        out = (bits, ok, iters[, post]) reuses caller arrays.  -> (bits[F,n], ok[F], iters[F][, post[F,n] float32]): post is the
        posterior LLR in natural-log units, and (post < 0, -0 included: np.signbit) is the word of every frame with ok = 1."""
        a = np.asarray(L)
        if a.dtype.kind not in "fiub":
            raise TypeError("decode_llr_batch takes real LLRs, not %s" % a.dtype)
        if a.ndim != 2:
            raise ValueError("L must be frames x n")
        a = np.ascontiguousarray(a, dtype=np.float32)
        with self._lease(H) as (h, code):
            if a.shape[1] != code.n:
                raise ValueError("L must be frames x n")
            F = a.shape[0]
            if out is not None:
                bits, ok, iters = out[:3]
                post = out[3] if posteriors else None
                assert bits.shape == (F, code.n) and bits.dtype == np.uint8 and bits.flags.c_contiguous
                assert ok.shape == (F,) and ok.dtype == np.uint8 and iters.shape == (F,) and iters.dtype == np.int32
                assert post is None or (post.shape == (F, code.n) and post.dtype == np.float32 and post.flags.c_contiguous)
            else:
                bits = np.empty((F, code.n), dtype=np.uint8)
                ok = np.empty(F, dtype=np.uint8)
                iters = np.empty(F, dtype=np.int32)
                post = np.empty((F, code.n), dtype=np.float32) if posteriors else None
            check(lib().acg_ldpc_decode_batch_llr(h, a.ctypes.data, F, bits.ctypes.data, ok.ctypes.data, iters.ctypes.data,
                                                  post.ctypes.data if post is not None else None))
        return (bits, ok, iters, post) if posteriors else (bits, ok, iters)

    def decode_llr_batch_dev(self, H, llr_ptr, frames, bits_ptr, ok_ptr, iters_ptr=None, post_ptr=None, stream=None):
        """device pointers (ints): frames*n float32 LLRs in; packed words, flags, iterations and, where post_ptr is given,
        frames*n float32 posteriors out; asynchronous on `stream` (None = the decoder's own stream)"""
        with self._lease(H) as (h, _):
            check(lib().acg_ldpc_decode_batch_llr_dev(h, llr_ptr, int(frames), bits_ptr, ok_ptr, iters_ptr, post_ptr, stream))


class StreamedLayeredBPDecoder(_StreamedLayered, BeliefPropagationDecoder):
    """Build-added (acg_ldpc_decoder_create_layered_streamed; not in the reference): layered sum-product — the reference's check
    rule, bp.h:49-57 — with fp32 posteriors and messages in device memory instead of LDS: one lane per frame, 4 n + 4 E bytes per
    frame, any code size and any check degree.  Word, flag and iteration of every frame equal those of
    BeliefPropagationDecoder(schedule=SCHEDULE_LAYERED, lanes_per_frame=256) on every code both accept, and a code whose frame
    fits in LDS is decoded faster there.  tests/layered_ref.py (layered_sumproduct_exact) restates it.  lanes_per_frame must stay
    0, precision PREC_DEFAULT and engine ENGINE_AUTO or ENGINE_STREAMED; not a stage of CascadeDecoder."""

    def __init__(self, max_iter, **kw):
        kw.setdefault("schedule", _lib.SCHEDULE_LAYERED)
        super().__init__(max_iter, **kw)


class StreamedLayeredMinSumDecoder(_StreamedLayered, MinSumDecoder):
    """Build-added: StreamedLayeredBPDecoder with the normalised min-sum check rule of MinSumDecoder(schedule=SCHEDULE_LAYERED,
    lanes_per_frame=256), equal to it frame for frame on every code both accept.  tests/layered_ref.py (layered_minsum)."""

    def __init__(self, max_iter, scale=1.0, **kw):
        kw.setdefault("schedule", _lib.SCHEDULE_LAYERED)
        super().__init__(max_iter, scale, **kw)


class OSDDecoder(Decoder):
    """Build-added ordered-statistics decoding of order 0 or 1 (algo = ACG_LDPC_OSD, include/acg_ldpc.h "OSD"; not in the
    reference): one GF(2) elimination per frame on int16 soft values, always a codeword (ok = 1), iters = candidates flipped
    (0 or 1).  Every value is an integer: tests/osd_ref.py restates it.  decode_batch quantises symbols (snr is ignored) and is
    weak on channel reliabilities alone; the intended use is CascadeDecoder(QuantizedMinSumDecoder(...), OSDDecoder(...)), which
    hands the first stage's posteriors over.  lanes_per_frame 0, 64, 128 or 256 = threads of the workgroup."""
    _algo = _lib.ALGO_OSD
    _name = "OSD"

    def __init__(self, order=1, lanes_per_frame=0, **kw):
        super().__init__(order, lanes_per_frame=lanes_per_frame, **kw)
        self.order = int(order)

    @staticmethod
    def soft_values(Y):
        """host symbols (float64, or float32) -> the int16 soft values the symbol entrance forms (acg_ldpc_debug_osd_soft)"""
        f32 = isinstance(Y, np.ndarray) and Y.dtype == np.float32
        Y = np.ascontiguousarray(Y, dtype=np.float32 if f32 else np.float64)
        out = np.empty(Y.shape, dtype=np.int16)
        check(lib().acg_ldpc_debug_osd_soft(Y.ctypes.data, 0 if f32 else 1, Y.size, out.ctypes.data))
        return out

    def decode_soft_batch(self, H, S):
        """S: frames x n INTEGER soft values (sign = hard decision, magnitude = reliability; every value must fit int16)
        -> (bits[F,n], ok[F], iters[F])"""
        a = np.asarray(S)
        if a.dtype.kind not in "iu":
            raise TypeError("decode_soft_batch takes integer soft values, not %s" % a.dtype)
        if a.dtype != np.int16:
            if a.size and (a.min() < -32768 or a.max() > 32767):
                raise ValueError("soft values must fit int16")
            a = a.astype(np.int16)
        a = np.ascontiguousarray(a)
        with self._lease(H) as (h, code):
            if a.ndim != 2 or a.shape[1] != code.n:
                raise ValueError("S must be frames x n")
            F = a.shape[0]
            bits = np.empty((F, code.n), dtype=np.uint8)
            ok = np.empty(F, dtype=np.uint8)
            iters = np.empty(F, dtype=np.int32)
            check(lib().acg_ldpc_osd_decode_batch(h, a.ctypes.data, F, bits.ctypes.data, ok.ctypes.data, iters.ctypes.data))
        return bits, ok, iters

    def decode_soft_batch_dev(self, H, s_ptr, frames, bits_ptr, ok_ptr, iters_ptr=None, stream=None):
        """device pointers (ints): frames*n int16 soft values in; packed words, flags and iters out; asynchronous on `stream`"""
        with self._lease(H) as (h, _):
            check(lib().acg_ldpc_osd_decode_batch_dev(h, s_ptr, int(frames), bits_ptr, ok_ptr, iters_ptr, stream))


class CascadeDecoder(_HandleCache):
    """Two-stage decoding (acg_ldpc_cascade_*): `first` decodes every frame, `second` only the frames `first` fails (ok = 0),
    from the same symbols — from the first's int16 posteriors where first is a QuantizedMinSumDecoder and second an OSDDecoder;
    the hand-over stays on the device.  first, second: Decoder objects as PARAMETER CARRIERS — their
    _params() and, for a QuantizedMinSumDecoder, their quantiser.  Their own handles are not borrowed: a cascade handle owns
    its two decoders, and this object caches cascade handles per H with the discipline of every Decoder.

        decode(H, channel_word, snr) -> (codeword, ok)
        decode_batch(H, Y, snr) -> (bits[F,n], ok[F], iters[F], stage[F])    stage: 1 or 2, the stage that produced the row
        name() -> "<first>+<second>", e.g. "MS+BP"
    """

    def __init__(self, first, second, max_handles=None):
        for d in (first, second):
            if not isinstance(d, Decoder):
                raise TypeError("CascadeDecoder takes two Decoder objects, not %s" % type(d).__name__)
        super().__init__(max_handles)
        self.first, self.second = first, second

    def _params(self):
        return self.first._params(), self.second._params()

    @staticmethod
    def _quant(d):
        return C.byref(d.quant.as_struct()) if isinstance(d, QuantizedMinSumDecoder) else None

    def _key(self, H):
        return super()._key(H) + tuple(("quant",) + d.quant.as_tuple() if isinstance(d, QuantizedMinSumDecoder) else ()
                                       for d in (self.first, self.second))

    def _create(self, code, p, h):
        return lib().acg_ldpc_cascade_create(code._h, C.byref(p[0]), self._quant(self.first), C.byref(p[1]),
                                             self._quant(self.second), C.byref(h))

    def _destroy(self, h):
        lib().acg_ldpc_cascade_destroy(h)

    def name(self):
        return self.first.name() + "+" + self.second.name()

    def stage_handle(self, H, stage):
        """the borrowed decoder handle of stage 0 / 1 of the cascade handle for H (acg_ldpc_cascade_stage): valid while that
        cascade handle lives; never destroy it"""
        h, _ = self.handle(H)
        s = lib().acg_ldpc_cascade_stage(h, int(stage))
        if not s:
            raise _lib.LdpcError(lib().acg_ldpc_last_error().decode())
        return C.c_void_p(s)

    def decode(self, H, channel_word, snr):
        bits, ok, _, stage = self.decode_batch(H, np.asarray(channel_word, dtype=np.float64)[None, :], snr)
        last = self.first if stage[0] == 1 else self.second
        if not ok[0] and last._algo != _lib.ALGO_QPADMM:
            return np.zeros(0, dtype=np.uint8), False  # {TCodeword(), false}, bp.h:198
        return bits[0], bool(ok[0])

    def decode_batch(self, H, Y, snr):
        """Y: frames x n channel symbols, float64 or float32 (travels as float32), as Decoder.decode_batch"""
        f32 = isinstance(Y, np.ndarray) and Y.dtype == np.float32
        Y = np.ascontiguousarray(Y, dtype=np.float32 if f32 else np.float64)
        with self._lease(H) as (h, code):
            if Y.ndim != 2 or Y.shape[1] != code.n:
                raise ValueError("Y must be frames x n")
            F = Y.shape[0]
            bits = np.empty((F, code.n), dtype=np.uint8)
            ok = np.empty(F, dtype=np.uint8)
            iters = np.empty(F, dtype=np.int32)
            stage = np.empty(F, dtype=np.uint8)
            fn = lib().acg_ldpc_cascade_decode_batch_f32 if f32 else lib().acg_ldpc_cascade_decode_batch
            check(fn(h, Y.ctypes.data, F, float(snr), bits.ctypes.data, ok.ctypes.data, iters.ctypes.data, stage.ctypes.data))
        return bits, ok, iters, stage

    def decode_batch_dev(self, H, y_ptr, y_is_f64, frames, snr, bits_ptr, ok_ptr, iters_ptr=None, stage_ptr=None, stream=None):
        """device pointers (ints); one host wait per chunk of 65536 frames, the tail asynchronous on `stream` (None = the
        first decoder's own stream)"""
        with self._lease(H) as (h, _):
            check(lib().acg_ldpc_cascade_decode_batch_dev(h, y_ptr, 1 if y_is_f64 else 0, int(frames), float(snr), bits_ptr,
                                                          ok_ptr, iters_ptr, stage_ptr, stream))

    def describe(self, H):
        """both stages' describe lines, the chunk and the last call's second-stage frames"""
        h, _ = self.handle(H)
        buf = C.create_string_buffer(4096)
        lib().acg_ldpc_cascade_describe(h, buf, 4096)
        return buf.value.decode()

    def last_call(self, H):
        """(frames handed to the second stage, device ms of the first decoder's launches, of the second's) of the most recent
        call on the handle for H; waits for the second stage's last launch"""
        h, _ = self.handle(H)
        k, a, b = C.c_int64(), C.c_float(), C.c_float()
        check(lib().acg_ldpc_cascade_last_call(h, C.byref(k), C.byref(a), C.byref(b)))
        return k.value, a.value, b.value
