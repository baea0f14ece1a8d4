"""What the tests of the quantiser grid (acg_ldpc_mc_run_quants / run_experiment_quants) share: tests/test_quant_grid.py on the
CPU, tests/test_quant_grid_gpu.py on the device.  Codes, SNRs and iteration counts are those of tests/layered_q_cases.py — the
smallest shapes that reach every path of bp_layered_q_kernel; this adds the list of points and the expectation.

POINTS: the three quantisers of layered_q_cases.QUANTS, a duplicate of the default, and four that differ from the default in one
respect each: a step whose inverse is no binary fraction, narrower channel values, narrower messages under wider posteriors, no
offset.  A kernel that read one point's quantiser for every frame, or the wrong row of the table, decodes some of them wrongly:
tests/test_quant_grid.py asserts that the restatement tells them apart.

ref_counters: the seven counters of a point from the restatement alone — the symbols host noise produces
(A.transmit_frames), decoded by layered_q_ref.layered_minsum_q, counted by mc_detail_ref.mc_detail."""
import numpy as np

import layered_q_cases as Q
import mc_detail_ref as R
from layered_q_ref import layered_minsum_q

DEFAULT = Q.QUANTS["default"]

# name -> (llr_step, ch_bits, msg_bits, post_bits, scale_num, scale_shift, offset), in the order the tests hand them over
POINTS = {
    "default": DEFAULT,
    "scaled": Q.QUANTS["scaled"],
    "saturating": Q.QUANTS["saturating"],
    "default again": DEFAULT,
    "step 0.3": (0.3,) + DEFAULT[1:],
    "ch_bits 4": (DEFAULT[0], 4) + DEFAULT[2:],
    "msg 5 post 10": DEFAULT[:2] + (5, 10) + DEFAULT[4:],
    "offset 0": DEFAULT[:6] + (0,),
}
assert len(POINTS) <= 8
NAMES = list(POINTS)
LIST = [POINTS[k] for k in NAMES]

FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")

FIRST, FRAMES = 5, 333      # where nothing else decides

_ref = {}


def sent(case, cws, first_frame, frames):
    """[frames, n] transmitted bits: frame g sends cws[g % len(cws)], the all-zero word where cws is None"""
    if cws is None:
        return np.zeros((frames, case.n), dtype=np.uint8)
    return np.asarray(cws)[(first_frame + np.arange(frames, dtype=np.int64)) % len(cws)]


def ref_counters(case, quant, first_frame, frames, cws, it=None):
    """the seven counters of global frames [first_frame, first_frame + frames) of `case` under `quant` (a 7-tuple) with host
    noise, as a tuple in the order of FIELDS; it: max_iter, the case's own by default.  Computed once per argument set."""
    import acg_alp_ldpc_amd as A
    it = case.iters if it is None else it
    key = (case.name, tuple(quant), first_frame, frames, it, None if cws is None else np.asarray(cws).tobytes())
    if key not in _ref:
        tx = np.zeros((1, case.n), dtype=np.uint8) if cws is None else cws
        y = A.transmit_frames(tx, case.snr, first_frame, frames)
        bits, ok, iters = layered_minsum_q(case.Hm, case.layers, y, case.snr, it, tuple(quant))
        c, _, _ = R.mc_detail(y, R.pack_bits(bits), ok, iters, sent(case, cws, first_frame, frames), case.Hm, first_frame=first_frame)
        _ref[key] = tuple(int(c[f]) for f in FIELDS)
    return _ref[key]


def counters(res):
    """an ExperimentResult -> the tuple ref_counters returns"""
    return tuple(int(getattr(res, f)) for f in FIELDS)


def case_words(case):
    """the codewords a test hands to the Monte-Carlo call for this case: its random ones (seven of them, so that frames cycle
    through the list), or None (the all-zero word) where the case has no generator"""
    return case.cws[:7] if case.cws.any() else None
