"""The frame sets on which the fp32 QP-ADMM kernels are held to tests/admm_ref.py — one definition for the CPU tests that
qualify the sets (tests/test_admm_ref.py: mutants visible, band census, early and late frames) and for the GPU tests that use
them (tests/test_admm_f32_exact_gpu.py).  Every restatement is computed once per FrameSets object and shared."""
import collections

import numpy as np

import admm_ref

FRAMES = 192
BUDGET = 60

# alpha, mu: the reference's parameters for its three matrices (main.cpp:31,33), those of the existing fp64 tests for the two
# synthetic codes
PARAMS = {"H05": (1.95, 0.5), "optimalH": (1.2, 0.55), "H": (1.9, 0.5), "mixed": (0.6, 1.0), "small": (0.6, 1.0),
          "regular": (1.95, 0.5)}
# optimalH again, close to its guard (e_min * mu = 2.2): a gain 1 / (mu * e - alpha) of 20 like H05's, with a mu whose
# products are inexact.  With (1.2, 0.55) the sweep is a contraction that forgets rounding differences.
HIGH_GAIN = (2.15, 0.55)

# codeword seed / first noise seed per (code, snr): chosen so that every set has frames that stop early and frames that run
# to the sweep limit (asserted in test_admm_ref.py)
SEEDS = {("H05", -2.0): (27, 27000), ("H05", 1.0): (27, 27000), ("optimalH", -2.0): (27, 27000), ("optimalH", 1.0): (11, 100),
         ("H", -2.0): (27, 27000), ("H", 1.0): (27, 27000), ("mixed", -2.0): (5, 300), ("small", -2.0): (5, 300),
         ("regular", 0.0): (5, 300)}

Set = collections.namedtuple("Set", "code snr alpha mu budget eps")


def make(code, snr, alpha=None, mu=None, budget=BUDGET, eps=1e-5):
    a, m = PARAMS[code]
    return Set(code, float(snr), a if alpha is None else alpha, m if mu is None else mu, budget, eps)


# the sets with the stopping rule on: each holds early and late frames, few banded ones
MAIN = [make(c, s) for c in ("H05", "optimalH", "H") for s in (-2.0, 1.0)]
EARLY_EXIT_SETS = MAIN + [make("optimalH", -2.0, *HIGH_GAIN), make("mixed", -2.0), make("small", -2.0, eps=1e-6),
                          make("regular", 0.0)]
# where a rounding difference in one operation survives to a word (gain 20): the mutants of test_admm_ref.py must show here.
# The other sets are there to reach kernel paths (one- and two-variable checks, list tails, pass counts): what goes wrong on
# those is structural — a wrong sign, a missed entry — and needs no sensitive frame.
SENSITIVE = [make("H05", -2.0), make("optimalH", -2.0, *HIGH_GAIN)]


def mixed_code():
    """the 230 x 400 code of test_qpadmm_mixed_check_degrees_and_long_lists: one- and two-variable checks next to long ones,
    variables in more checks than the register-resident list of the workgroup-per-frame kernel holds"""
    rng = np.random.default_rng(11)
    m, n = 230, 400
    H = np.zeros((m, n), np.uint8)
    degs = rng.choice([1, 2, 3, 4, 5, 6, 8], size=m, p=[0.08, 0.12, 0.2, 0.2, 0.2, 0.1, 0.1])
    for i, d in enumerate(degs):
        H[i, rng.choice(n, size=d, replace=False)] = 1
    H[:9, 3] = 1
    H[20:32, 5] = 1
    for v in np.nonzero(H.sum(0) == 0)[0]:
        H[rng.integers(40, m), v] = 1
    return H


def small_code():
    """the 5 x 8 code of test_qpadmm_guard_and_small_checks: checks of one, two, three and five variables"""
    H = np.zeros((5, 8), np.uint8)
    H[0, [0, 1, 2, 3, 4]] = 1
    H[1, [2, 5]] = 1
    H[2, [6]] = 1
    H[3, [1, 3, 7]] = 1
    H[4, [0, 7]] = 1
    return H


def regular_code():
    """(3,6)-regular 200 x 400: 800 constraint groups, more than the 64-lane kernel keeps in registers (12 per lane)"""
    from acg_alp_ldpc_amd.codes import regular_ldpc
    return np.asarray(regular_ldpc(200, 400, 3, 6, seed=1), dtype=np.uint8)


class FrameSets:
    def __init__(self, oracle, matrices):
        self.oracle = oracle
        self.H = dict(matrices)
        self.H["mixed"] = mixed_code()
        self.H["small"] = small_code()
        self.H["regular"] = regular_code()
        self._problem, self._frames, self._ref = {}, {}, {}

    def problem(self, code):
        if code not in self._problem:
            self._problem[code] = admm_ref.admm_problem(self.H[code])
        return self._problem[code]

    def band(self, code):
        return admm_ref.band_width(len(self.problem(code)[3]))

    def frames(self, code, snr):
        """(codewords, float64 symbols) of the set: oracle.gen_codewords through oracle.transmit_frames"""
        k = (code, float(snr))
        if k not in self._frames:
            G, ok = self.oracle.get_orthogonal(self.H[code])
            assert ok
            cw_seed, first = SEEDS[k]
            cws = self.oracle.gen_codewords(G, cw_seed, FRAMES)
            self._frames[k] = (cws, self.oracle.transmit_frames(cws, snr, first_seed=first))
        return self._frames[k]

    def ref(self, s, dtype=np.float32, y=None, tag=None, mutant=None):
        """the restatement of set s -> (bits, ok, iters, band); y (with a tag naming it) replaces the set's own symbols"""
        k = (s, np.dtype(dtype).name, tag, mutant)
        assert (y is None) == (tag is None)
        if k not in self._ref:
            if y is None:
                y = self.frames(s.code, s.snr)[1]
            self._ref[k] = admm_ref.qpadmm_ref(self.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, s.eps, dtype,
                                               problem=self.problem(s.code), mutant=mutant)
        return self._ref[k]

    def clear(self, s, band):
        """frames on which a kernel must equal the restatement: all of them without the stopping rule, else those whose
        residual never came within the band of eps"""
        if s.eps <= 0:
            return np.ones(len(band), dtype=bool)
        return band >= self.band(s.code)
