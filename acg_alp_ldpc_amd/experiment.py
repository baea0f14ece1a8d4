"""Monte-Carlo harness: the reference's experiment.h (ExperimentResult, multithread_experiment,
merge_exp_results) with the frame loop on the GPU.

Sharding: frames are independent, so rank r of W simulates the contiguous global
range [r*F/W, (r+1)*F/W); noise seeds derive from the GLOBAL frame index, so the union of the
shards is the same set of frames for any W.  The only cross-rank step is adding seven integers
(merge_exp_results, experiment.h:70-78) — no data-path collective.
"""
import ctypes as C
import threading
import time

import numpy as np

from . import _lib
from ._lib import McCfg, McDetail, McResult, check, lib


class ExperimentResult:
    """experiment.h:49-68 (+ sum_iters / kernel_ms for the throughput report)"""
    FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, int(kw.get(f, 0)))
        self.time_sec = float(kw.get("time_sec", 0.0))
        self.kernel_ms = float(kw.get("kernel_ms", 0.0))

    def FER(self):
        return (self.total - self.correct) / self.total

    def avg_time(self):
        return self.time_sec / self.total

    def mean_hamming(self):
        return self.sum_hamming / self.total

    def mean_hamming_ok(self):
        return self.sum_hamming_ok / max(1, self.correct)

    def mean_hamming_wrong(self):
        return self.sum_hamming_wrong / max(1, self.total - self.correct)

    def mean_iters(self):
        return self.sum_iters / max(1, self.total)

    def as_vector(self):
        return np.array([getattr(self, f) for f in self.FIELDS], dtype=np.int64)

    @classmethod
    def from_vector(cls, v, time_sec=0.0, kernel_ms=0.0):
        return cls(time_sec=time_sec, kernel_ms=kernel_ms, **{f: int(x) for f, x in zip(cls.FIELDS, v)})

    def __repr__(self):
        return "ExperimentResult(" + ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS) + ")"


def merge_exp_results(a, b):
    """experiment.h:70-78"""
    for f in ExperimentResult.FIELDS:
        setattr(a, f, getattr(a, f) + getattr(b, f))
    a.time_sec += b.time_sec
    a.kernel_ms += b.kernel_ms
    return a


def shard_range(frames, rank, world):
    """contiguous global frame range of `rank`"""
    lo = (frames * rank) // world
    hi = (frames * (rank + 1)) // world
    return lo, hi - lo


def run_experiment(decoder, codewords, H, snr, frames=None, first_frame=0, noise="host", seed=1):
    """multithread_experiment (experiment.h:125-139) for global frames [first_frame, first_frame+frames).

    noise="host":   bit-exact reference frames (frame g <- mt19937(g+1), libstdc++ normal_distribution);
                    frame g transmits codewords[g % len(codewords)] (the reference: one codeword per frame).
    noise="device": Philox AWGN generated inside the decode kernel (throughput runs).
    codewords=None: the all-zero codeword.
    """
    h, code = decoder.handle(H)
    cfg = McCfg()
    cw = None
    if codewords is not None:
        cw = np.ascontiguousarray(codewords, dtype=np.uint8)
        assert cw.ndim == 2 and cw.shape[1] == code.n
        cfg.codewords = cw.ctypes.data
        cfg.n_codewords = cw.shape[0]
    if frames is None:
        if cw is None:
            raise ValueError("frames required without codewords")
        frames = cw.shape[0]
    cfg.frames = int(frames)
    cfg.first_frame = int(first_frame)
    cfg.snr = float(snr)
    cfg.seed = int(seed)
    cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
    res = McResult()
    check(lib().acg_ldpc_mc_run(h, C.byref(cfg), C.byref(res)))
    return ExperimentResult(**{f: getattr(res, f) for f in ExperimentResult.FIELDS}, time_sec=res.time_sec,
                            kernel_ms=res.kernel_ms)


def _index_list(n, idx, what):
    idx = np.asarray(list(idx), dtype=np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("rate_match_pattern: %s index %d is outside 0 ... %d" % (what, int(idx[(idx < 0) | (idx >= n)][0]), n - 1))
    return idx


def rate_match_pattern(n, punctured=(), shortened=()):
    """The pattern of acg_ldpc_mc_run_rm: uint8 [n], _lib.RM_PUNCTURED at the punctured indices, _lib.RM_SHORTENED at the
    shortened ones, _lib.RM_SENT elsewhere.  An index in both lists, or outside 0 ... n - 1, is a ValueError."""
    n = int(n)
    p, s = _index_list(n, punctured, "punctured"), _index_list(n, shortened, "shortened")
    both = np.intersect1d(p, s)
    if both.size:
        raise ValueError("rate_match_pattern: index %d is both punctured and shortened" % int(both[0]))
    pat = np.zeros(n, dtype=np.uint8)
    pat[p] = _lib.RM_PUNCTURED
    pat[s] = _lib.RM_SHORTENED
    return pat


def _pattern_bytes(pattern, n):
    """pattern (None = all sent) as the contiguous uint8 [n] the C calls read; values outside a byte are refused here"""
    if pattern is None:
        return None
    a = np.asarray(pattern)
    if a.shape != (n,):
        raise ValueError("pattern must have n = %d entries" % n)
    if a.dtype.kind not in "iub" or (a.size and (a.min() < 0 or a.max() > 255)):
        raise ValueError("pattern entries are _lib.RM_SENT, RM_PUNCTURED or RM_SHORTENED")
    return np.ascontiguousarray(a, dtype=np.uint8)


def run_experiment_rm(decoder, codewords, H, snr, pattern=None, frames=None, first_frame=0, seed=1):
    """acg_ldpc_mc_run_rm: run_experiment with device noise for a punctured / shortened code.  pattern: uint8 [n] as
    rate_match_pattern returns it (None: every position sent).  A punctured position reaches the decoder as an erasure, a
    shortened one as a known bit; raw errors are counted over the sent positions; a frame is correct when the word equals the
    sent one on all n positions.  snr is Es/N0 of a transmitted symbol.  decoder: a StreamedLayeredBPDecoder,
    StreamedLayeredMinSumDecoder, QuantizedMinSumDecoder or StreamedQuantizedMinSumDecoder (the engines with a channel-value
    entrance); the library refuses every other.  Other arguments as run_experiment."""
    from .code import ParityCheckMatrix
    pat = _pattern_bytes(pattern, H.n if isinstance(H, ParityCheckMatrix) else np.asarray(H).shape[1])   # (before a handle is made)
    with decoder._lease(H) as (h, code):
        cfg = McCfg()
        cw = None
        if codewords is not None:
            cw = np.ascontiguousarray(codewords, dtype=np.uint8)
            assert cw.ndim == 2 and cw.shape[1] == code.n
            cfg.codewords = cw.ctypes.data
            cfg.n_codewords = cw.shape[0]
        if frames is None:
            if cw is None:
                raise ValueError("frames required without codewords")
            frames = cw.shape[0]
        cfg.frames = int(frames)
        cfg.first_frame = int(first_frame)
        cfg.snr = float(snr)
        cfg.seed = int(seed)
        cfg.noise = _lib.NOISE_DEVICE_PHILOX
        res = McResult()
        check(lib().acg_ldpc_mc_run_rm(h, C.byref(cfg), None if pat is None else pat.ctypes.data, C.byref(res)))
    return ExperimentResult(**{f: getattr(res, f) for f in ExperimentResult.FIELDS}, time_sec=res.time_sec,
                            kernel_ms=res.kernel_ms)


CASCADE_EXTRAS = ("second_frames", "second_correct", "second_pseudo", "second_sum_iters", "second_kernel_ms")


def run_experiment_cascade(cascade, codewords, H, snr, frames=None, first_frame=0, noise="host", seed=1):
    """acg_ldpc_cascade_mc_run: run_experiment through a CascadeDecoder.  Returns (total, first, extras): the ExperimentResult
    of the returned outputs, the ExperimentResult of the first decoder alone on the same frames (its seven counters are
    run_experiment's on that decoder), and a dict of the second stage's figures (CASCADE_EXTRAS): the frames handed to it, how
    many of them it decoded correctly / to a pseudo-codeword, its sweeps and its device time.  Arguments as run_experiment."""
    with cascade._lease(H) as (h, code):
        cfg = McCfg()
        cw = None
        if codewords is not None:
            cw = np.ascontiguousarray(codewords, dtype=np.uint8)
            assert cw.ndim == 2 and cw.shape[1] == code.n
            cfg.codewords = cw.ctypes.data
            cfg.n_codewords = cw.shape[0]
        if frames is None:
            if cw is None:
                raise ValueError("frames required without codewords")
            frames = cw.shape[0]
        cfg.frames = int(frames)
        cfg.first_frame = int(first_frame)
        cfg.snr = float(snr)
        cfg.seed = int(seed)
        cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
        res = _lib.CascadeResult()
        check(lib().acg_ldpc_cascade_mc_run(h, C.byref(cfg), C.byref(res)))
    total, first = (ExperimentResult(**{f: getattr(r, f) for f in ExperimentResult.FIELDS}, time_sec=r.time_sec,
                                     kernel_ms=r.kernel_ms) for r in (res.total, res.first))
    return total, first, {f: getattr(res, f) for f in CASCADE_EXTRAS}


def merge_cascade_results(a, b):
    """acg_ldpc_cascade_merge for shards, on the triples run_experiment_cascade returns: everything adds.  a is updated and returned."""
    merge_exp_results(a[0], b[0])
    merge_exp_results(a[1], b[1])
    for f in CASCADE_EXTRAS:
        a[2][f] += b[2][f]
    return a


# acg_ldpc_mc_event as a numpy record (32 bytes)
EVENT_DTYPE = np.dtype([("frame", "<i8"), ("kind", "<i4"), ("iters", "<i4"), ("raw_errors", "<i4"), ("bit_errors", "<i4"),
                        ("syndrome_weight", "<i4"), ("reserved", "<i4")])


class ExperimentDetail(ExperimentResult):
    """acg_ldpc_mc_detail: ExperimentResult plus the bit errors of the returned words, the frames that are not correct split
    by kind (_lib.EVENT_*), and the first `cap` of them in ascending global frame order.

    events: numpy structured array (EVENT_DTYPE), n_stored entries.  words: uint32[n_stored, (n+31)//32], row k = returned
    word XOR sent word of event k (all-zero for an EVENT_NO_WORD), or None when the run did not ask for them.
    A frame without a returned word (BP out of iterations, QP-ADMM guard) adds nothing to bit_errors: BER() is the bit
    error rate over returned words — undetected errors for BP, all bit errors for QP-ADMM."""
    DETAIL_FIELDS = ("word_frames", "bit_errors", "noncodeword_frames", "sum_syndrome_weight", "n_events", "n_stored")

    def __init__(self, n=0, cap=0, events=None, words=None, **kw):
        super().__init__(**kw)
        for f in self.DETAIL_FIELDS:
            setattr(self, f, int(kw.get(f, 0)))
        self.min_pseudo_weight = int(kw.get("min_pseudo_weight", -1))
        self.min_pseudo_frame = int(kw.get("min_pseudo_frame", -1))
        self.n = int(n)
        self.cap = int(cap)
        self.events = np.zeros(0, dtype=EVENT_DTYPE) if events is None else events
        self.words = words

    def BER(self):
        """bit errors of the returned words over ALL transmitted bits (total * n)"""
        return self.bit_errors / (self.total * self.n)

    def BER_returned(self):
        """the same per returned word: bit_errors / (word_frames * n)"""
        return self.bit_errors / max(1, self.word_frames * self.n)

    def mean_syndrome_weight(self):
        return self.sum_syndrome_weight / max(1, self.noncodeword_frames)

    def __repr__(self):
        return "ExperimentDetail(" + ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS + self.DETAIL_FIELDS +
                                               ("min_pseudo_weight", "min_pseudo_frame")) + ")"


def merge_exp_details(a, b):
    """acg_ldpc_mc_detail_merge for shards: counters add, the smaller min_pseudo_weight wins (-1 = none; tie: the lower
    frame), the event lists are concatenated, sorted by frame and cut to a.cap."""
    merge_exp_results(a, b)
    for f in ("word_frames", "bit_errors", "noncodeword_frames", "sum_syndrome_weight", "n_events"):
        setattr(a, f, getattr(a, f) + getattr(b, f))
    if b.min_pseudo_weight > 0 and (a.min_pseudo_weight <= 0 or (b.min_pseudo_weight, b.min_pseudo_frame) <
                                    (a.min_pseudo_weight, a.min_pseudo_frame)):
        a.min_pseudo_weight, a.min_pseudo_frame = b.min_pseudo_weight, b.min_pseudo_frame
    if a.min_pseudo_weight <= 0:
        a.min_pseudo_weight, a.min_pseudo_frame = -1, -1
    a.n = a.n or b.n
    ev = np.concatenate([a.events, b.events])
    order = np.argsort(ev["frame"], kind="stable")[:a.cap]
    if a.words is not None and b.words is not None:
        a.words = np.concatenate([a.words, b.words])[order]
    else:
        a.words = None
    a.events = ev[order]
    a.n_stored = len(a.events)
    return a


def run_experiment_detail(decoder, codewords, H, snr, frames=None, first_frame=0, noise="host", seed=1, cap=0, words=False):
    """acg_ldpc_mc_run_detail: run_experiment plus post-decoding bit errors and a log of the frames that are not correct.

    cap: how many events to store — those of the cap lowest global frame indices, whatever the launch shape.
    words=True: also return word XOR sent for every stored event.  Other arguments as run_experiment.
    Returns an ExperimentDetail."""
    h, code = decoder.handle(H)
    cfg = McCfg()
    cw = None
    if codewords is not None:
        cw = np.ascontiguousarray(codewords, dtype=np.uint8)
        assert cw.ndim == 2 and cw.shape[1] == code.n
        cfg.codewords = cw.ctypes.data
        cfg.n_codewords = cw.shape[0]
    if frames is None:
        if cw is None:
            raise ValueError("frames required without codewords")
        frames = cw.shape[0]
    cfg.frames = int(frames)
    cfg.first_frame = int(first_frame)
    cfg.snr = float(snr)
    cfg.seed = int(seed)
    cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
    cap = int(cap)
    nwords = (code.n + 31) // 32
    ev = np.zeros(max(cap, 0), dtype=EVENT_DTYPE)
    wd = np.zeros((max(cap, 0), nwords), dtype=np.uint32) if words else None
    res = McDetail()
    check(lib().acg_ldpc_mc_run_detail(h, C.byref(cfg), C.byref(res), ev.ctypes.data if cap > 0 else None,
                                       wd.ctypes.data if (wd is not None and cap > 0) else None, cap))
    return detail_from_struct(res, code.n, cap, ev, wd)


def detail_from_struct(res, n, cap, events, words):
    """ExperimentDetail of a filled _lib.McDetail and the buffers the call wrote"""
    kw = {f: getattr(res.base, f) for f in ExperimentResult.FIELDS}
    kw.update({f: getattr(res, f) for f in ExperimentDetail.DETAIL_FIELDS})
    ns = int(res.n_stored)
    return ExperimentDetail(n=n, cap=cap, events=events[:ns].copy(), words=None if words is None else words[:ns].copy(),
                            time_sec=res.base.time_sec, kernel_ms=res.base.kernel_ms, min_pseudo_weight=res.min_pseudo_weight,
                            min_pseudo_frame=res.min_pseudo_frame, **kw)


def run_experiment_grid(decoder, codewords, H, snr, alphas, mus, frames=None, first_frame=0, noise="host", seed=1):
    """The (alpha, mu) loop of qpadmm_params.cpp:64-77 in one call on one handle (acg_ldpc_mc_run_grid): point k decodes
    the same frames as every other point with (alphas[k], mus[k]) in place of the decoder's own alpha and mu.

    decoder: a QPADMMDecoder; its max_iter, eps_stop, early_exit, precision and engine apply.  Returns one
    ExperimentResult per point, equal to run_experiment on QPADMMDecoder(alphas[k], mus[k], ...) except that guard
    points (e_min*mu <= alpha) are counted as failures instead of refused, time_sec is the wall time of the whole call
    and kernel_ms the point's share of device time.  Other arguments as run_experiment."""
    a = np.ascontiguousarray(alphas, dtype=np.float64).ravel()
    m = np.ascontiguousarray(mus, dtype=np.float64).ravel()
    if a.shape != m.shape:
        raise _lib.LdpcError("run_experiment_grid: alphas and mus must have the same length (%d != %d)" % (a.size, m.size))
    with decoder._lease(H) as (h, code):
        cfg = McCfg()
        cw = None
        if codewords is not None:
            cw = np.ascontiguousarray(codewords, dtype=np.uint8)
            assert cw.ndim == 2 and cw.shape[1] == code.n
            cfg.codewords = cw.ctypes.data
            cfg.n_codewords = cw.shape[0]
        if frames is None:
            if cw is None:
                raise ValueError("frames required without codewords")
            frames = cw.shape[0]
        cfg.frames = int(frames)
        cfg.first_frame = int(first_frame)
        cfg.snr = float(snr)
        cfg.seed = int(seed)
        cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
        res = (McResult * max(1, a.size))()
        check(lib().acg_ldpc_mc_run_grid(h, C.byref(cfg), a.ctypes.data, m.ctypes.data, int(a.size), res))
    return [ExperimentResult(**{f: getattr(r, f) for f in ExperimentResult.FIELDS}, time_sec=r.time_sec,
                             kernel_ms=r.kernel_ms) for r in res[:a.size]]


def quant_structs(quants):
    """a sequence of QuantConfig, 7-tuples (llr_step, ch_bits, msg_bits, post_bits, scale_num, scale_shift, offset) or dicts of
    QuantConfig's fields (the others at their defaults) -> a ctypes array of _lib.Quant, at least one entry long"""
    from .decoder import QuantConfig
    out = (_lib.Quant * max(1, len(quants)))()
    for k, q in enumerate(quants):
        if isinstance(q, dict):
            q = QuantConfig(**q)
        elif not isinstance(q, QuantConfig):
            q = tuple(q)
            if len(q) != 7:
                raise _lib.LdpcError("run_experiment_quants: quants[%d] has %d values, a quantiser has 7" % (k, len(q)))
            q = QuantConfig(*q)
        out[k] = q.as_struct()
    return out


def run_experiment_quants(decoder, codewords, H, snr, quants, frames=None, first_frame=0, noise="host", seed=1):
    """The format search of the fixed-point layered min-sum engine in one call on one handle (acg_ldpc_mc_run_quants): point k
    decodes the same frames as every other point with quants[k] in place of the decoder's own quantiser.

    decoder: a QuantizedMinSumDecoder; its max_iter, early_exit and lanes_per_frame apply.  quants: QuantConfig, 7-tuples or
    dicts (quant_structs).  Returns one ExperimentResult per point, equal in the seven counters to run_experiment on
    QuantizedMinSumDecoder(..., quant=quants[k]); time_sec is the wall time of the whole call and kernel_ms the point's share
    of device time.  An invalid quantiser anywhere in the list is refused (LdpcError naming its index).  Other arguments as
    run_experiment."""
    from .decoder import QuantizedMinSumDecoder
    if not isinstance(decoder, QuantizedMinSumDecoder):
        raise _lib.LdpcError("run_experiment_quants needs a QuantizedMinSumDecoder (acg_ldpc_decoder_create_quantized)")
    quants = list(quants)
    qs = quant_structs(quants)
    with decoder._lease(H) as (h, code):
        cfg = McCfg()
        cw = None
        if codewords is not None:
            cw = np.ascontiguousarray(codewords, dtype=np.uint8)
            assert cw.ndim == 2 and cw.shape[1] == code.n
            cfg.codewords = cw.ctypes.data
            cfg.n_codewords = cw.shape[0]
        if frames is None:
            if cw is None:
                raise ValueError("frames required without codewords")
            frames = cw.shape[0]
        cfg.frames = int(frames)
        cfg.first_frame = int(first_frame)
        cfg.snr = float(snr)
        cfg.seed = int(seed)
        cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
        res = (McResult * max(1, len(quants)))()
        check(lib().acg_ldpc_mc_run_quants(h, C.byref(cfg), qs, len(quants), res))
    return [ExperimentResult(**{f: getattr(r, f) for f in ExperimentResult.FIELDS}, time_sec=r.time_sec,
                             kernel_ms=r.kernel_ms) for r in res[:len(quants)]]


class CodesEvaluator:
    """acg_ldpc_evaluator: scores batches of parity-check matrices of one m x n under one set of QP-ADMM parameters
    (the scoring of optimize_H.cpp:16-25 for many proposals at once).  params_or_decoder: a QPADMMDecoder (its alpha, mu,
    max_iter, eps_stop, early_exit, precision, lanes_per_frame and engine apply) or a _lib.Params."""

    def __init__(self, params_or_decoder):
        p = params_or_decoder if isinstance(params_or_decoder, _lib.Params) else params_or_decoder._params()
        self._h = C.c_void_p()
        check(lib().acg_ldpc_evaluator_create(C.byref(p), C.byref(self._h)))

    def run(self, codes, snr, frames=None, first_frame=0, noise="host", seed=1):
        """codes: a list of (H, codewords); H a ParityCheckMatrix or a dense 0/1 matrix, codewords an array of that code's own
        words (None: the all-zero word).  Returns one ExperimentResult per code, equal in the seven counters to run_experiment
        on that code's own QPADMMDecoder(..., fast_setup=True); guard codes (e_min*mu <= alpha) are counted as failures."""
        from .code import ParityCheckMatrix
        pcms, cws = [], []
        cfgs = (McCfg * max(1, len(codes)))()
        for k, (H, cw) in enumerate(codes):
            code = H if isinstance(H, ParityCheckMatrix) else ParityCheckMatrix(H)
            pcms.append(code)
            cfg = cfgs[k]
            if cw is not None:
                cw = np.ascontiguousarray(cw, dtype=np.uint8)
                if cw.ndim != 2 or cw.shape[1] != code.n:
                    raise ValueError("codewords must be count x n")
                cfg.codewords = cw.ctypes.data
                cfg.n_codewords = cw.shape[0]
            cws.append(cw)  # (keeps the array alive for the call)
            f = frames
            if f is None:
                if cw is None:
                    raise ValueError("frames required without codewords")
                f = cw.shape[0]
            cfg.frames = int(f)
            cfg.first_frame = int(first_frame)
            cfg.snr = float(snr)
            cfg.seed = int(seed)
            cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
        handles = (C.c_void_p * max(1, len(pcms)))(*[c._h.value for c in pcms])
        res = (McResult * max(1, len(pcms)))()
        check(lib().acg_ldpc_mc_run_codes(self._h, handles, len(pcms), cfgs, res))
        return [ExperimentResult(**{f: getattr(r, f) for f in ExperimentResult.FIELDS}, time_sec=r.time_sec,
                                 kernel_ms=r.kernel_ms) for r in res[:len(pcms)]]

    def describe(self):
        """one line on what the last run did: mc_codes=single-launch groups=<g> chunks=<c> ... or mc_codes=per-code ..."""
        buf = C.create_string_buffer(512)
        lib().acg_ldpc_evaluator_describe(self._h, buf, 512)
        return buf.value.decode()

    def close(self):
        if self._h:
            lib().acg_ldpc_evaluator_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_experiment_codes(params_or_decoder, codes, snr, frames=None, first_frame=0, noise="host", seed=1):
    """acg_ldpc_mc_run_codes: run_experiment for every (H, codewords) of `codes` in one call — the codes the
    workgroup-per-frame QP-ADMM kernel accepts share one launch per launch shape.  params_or_decoder: a QPADMMDecoder, a
    _lib.Params, or a CodesEvaluator to reuse (its buffers stay).  See CodesEvaluator.run."""
    if isinstance(params_or_decoder, CodesEvaluator):
        return params_or_decoder.run(codes, snr, frames, first_frame, noise, seed)
    ev = CodesEvaluator(params_or_decoder)
    try:
        return ev.run(codes, snr, frames, first_frame, noise, seed)
    finally:
        ev.close()


def run_experiment_sharded(decoder, codewords, H, snr, frames, rank=0, world=1, noise="device", seed=1, group=None):
    """One rank's shard + host-side sum of the counters across ranks.

    With world > 1, torch.distributed must be initialised (gloo or nccl); the all_reduce carries
    seven integers and is control-plane only."""
    lo, cnt = shard_range(int(frames), rank, world)
    t0 = time.time()
    local = run_experiment(decoder, codewords, H, snr, frames=cnt, first_frame=lo, noise=noise, seed=seed)
    if world == 1:
        return local, local
    import torch
    import torch.distributed as dist
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    v = torch.from_numpy(local.as_vector()).to(dev)
    dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
    total = ExperimentResult.from_vector(v.cpu().numpy(), time_sec=time.time() - t0, kernel_ms=local.kernel_ms)
    return local, total


def run_experiment_inproc(make_decoder, codewords, H, snr, frames, devices, noise="device", seed=1):
    """All GPUs of a node from ONE process, no torch.distributed: one host thread and one decoder per device (what
    multithread_experiment does with pthreads, experiment.h:125-139), shard g = the contiguous global range
    shard_range(frames, g, len(devices)), counters merged on the host (merge_exp_results, experiment.h:70-78).

    make_decoder(device) -> a Decoder bound to that device.  Returns (per-shard results, merged total)."""
    devices = list(devices)
    W = len(devices)
    locals_ = [None] * W
    errs = []

    def work(g):
        try:
            dec = make_decoder(devices[g])
            lo, cnt = shard_range(int(frames), g, W)
            locals_[g] = run_experiment(dec, codewords, H, snr, frames=cnt, first_frame=lo, noise=noise, seed=seed)
        except Exception as e:  # noqa: BLE001 - re-raised below in the calling thread
            errs.append(e)

    t0 = time.time()
    th = [threading.Thread(target=work, args=(g,)) for g in range(W)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise errs[0]
    total = ExperimentResult()
    for r in locals_:
        merge_exp_results(total, r)
    total.time_sec = time.time() - t0
    return locals_, total
