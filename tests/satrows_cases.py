"""The batch that drives the edge rows of the fused sum-product sweeps through phi's end cases, shared by tests/test_satrows.py
(which checks on the CPU, with the census model, what the rows without a fast-path test meet) and tests/test_satrows_gpu.py (which
decodes it with the specialised and with the generic instance).  Symbols of the all-zero codeword, NumPy only."""
import numpy as np

END_SNR = -2.0
END_FRAMES = 64


def end_case_batch(n):
    """64 frames x n float64 channel symbols at END_SNR:
       0-15  symbols scaled by 64 with magnitudes of 0.5 and more before: every |LLR| >= 66 (phi gives +0, the checks then see +0)
      16-23  all-zero symbols (phi(0) = +inf on the variable side, +inf into the checks)
      24-47  noisy frames with a single symbol set to +inf or -inf
      48-55  noisy frames with one NaN symbol
      56-63  noisy frames scaled by 2^-20 (phi of such an LLR is about 20, so a check's exclude-self sums pass 66 while finite) with
             a single symbol set to +inf or -inf"""
    rng = np.random.RandomState(1515)
    sigma = np.sqrt(10 ** (-END_SNR / 10) / 2)
    y = 1.0 + sigma * rng.standard_normal((END_FRAMES, n))
    big = np.sign(y[:16]) * np.maximum(np.abs(y[:16]), 0.5) * 64.0
    y[:16] = big
    y[16:24] = 0.0
    for f in range(24, 48):
        y[f, (37 * f) % n] = np.inf if f % 2 else -np.inf
    for f in range(48, 56):
        y[f, (53 * f) % n] = np.nan
    y[56:64] *= 2.0 ** -20
    for f in range(56, 64):
        y[f, (29 * f) % n] = np.inf if f % 2 else -np.inf
    return np.ascontiguousarray(y, dtype=np.float64)
