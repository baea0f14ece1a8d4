"""The phi fast-path tests as a per-row property of a build-time instance (bp_core.inc: c_sat_rows / v_sat_rows of a static pass
policy; masks from the generator's census): a row without its test evaluates phi where the test would have supplied the value,
on the same bits, so every output and every device counter equals that of the generic instance, which keeps every test and which
a handle created under ACG_BP_NO_SPEC=1 runs.  One case per entry of the default SPEC_CODES, selected as tests/test_spec_gpu.py
does.  The end-case batch is tests/satrows_cases.py's; tests/test_satrows.py checks on the CPU what it drives the cleared rows
through.  Run with `-m gpu` on an MI355X."""
import contextlib
import os
import re

import numpy as np
import pytest

import acg_alp_ldpc_amd as A
from satrows_cases import END_SNR, end_case_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"H05_L32": "H05", "H_L64": "H", "optimalH_L32": "optimalH"}
SNRS = (-3.0, -2.0, 2.0)
FRAMES = (1, 7, 2003)      # 7: less than one chunk of 8 frames
MAX_ITERS = (0, 1, 2, 50)


@contextlib.contextmanager
def no_spec(on):
    old = os.environ.pop("ACG_BP_NO_SPEC", None)
    if on:
        os.environ["ACG_BP_NO_SPEC"] = "1"
    try:
        yield
    finally:
        os.environ.pop("ACG_BP_NO_SPEC", None)
        if old is not None:
            os.environ["ACG_BP_NO_SPEC"] = old


def decoder(H, generic, max_iter=50):
    d = A.BeliefPropagationDecoder(max_iter, early_exit=False)
    with no_spec(generic):
        text = d.describe(H)
    return d, text


@pytest.fixture(scope="module", params=sorted(ENTRIES))
def entry(request):
    """per entry: name, H, codewords, per SNR the symbols of the largest batch and the end-case batch, made once and left alone"""
    from oracle.pyoracle import Oracle
    name = request.param
    Hm = Oracle().read_pcm(os.path.join(ROOT, "data", ENTRIES[name] + ".txt"))
    H = A.ParityCheckMatrix(Hm)
    G, ok = H.get_orthogonal()
    assert ok
    cws = A.gen_random_codewords(G, 64, 1515)
    y = {snr: A.transmit_frames(cws[np.arange(max(FRAMES)) % len(cws)], snr) for snr in SNRS}
    return name, H, cws, y, end_case_batch(Hm.shape[1])


def pair(name, H, max_iter=50):
    spec, t_spec = decoder(H, False, max_iter)
    gen, t_gen = decoder(H, True, max_iter)
    assert t_spec.endswith(" spec=" + name) and t_gen.endswith(" spec=0"), (t_spec, t_gen)
    # the masks stand next to the instance's name, with the census they come from; the generic instance has none
    assert re.search(r" sat_rows=c:[0-9a-f,]+/v:[0-9a-f,]+@-?[0-9.]+dB,t[0-9.]+ spec=", t_spec) and "sat_rows" not in t_gen, (t_spec, t_gen)
    return spec, gen


def same(a, b, *what):
    for k, part in enumerate(("bits", "ok", "iters")):
        assert a[k].tobytes() == b[k].tobytes(), what + (part, int((a[k] != b[k]).sum()))


def test_outputs_equal_the_generic_instance(entry):
    name, H, _, y, _ = entry
    for max_iter in MAX_ITERS:
        spec, gen = pair(name, H, max_iter)
        for snr in SNRS:
            for frames in FRAMES:
                same(spec.decode_batch(H, y[snr][:frames], snr), gen.decode_batch(H, y[snr][:frames], snr), name, max_iter, snr, frames)
        spec.close()
        gen.close()


def test_end_cases_equal_the_generic_instance(entry):
    name, H, _, _, yend = entry
    for max_iter in MAX_ITERS:
        spec, gen = pair(name, H, max_iter)
        same(spec.decode_batch(H, yend, END_SNR), gen.decode_batch(H, yend, END_SNR), name, max_iter, "end cases")
        spec.close()
        gen.close()


def test_freeze_and_monte_carlo_counters_equal(entry):
    name, H, cws, y, _ = entry
    spec, gen = pair(name, H)
    assert spec.freeze_stats(H) == (0, 0) and gen.freeze_stats(H) == (0, 0)   # counting on from here
    for snr in SNRS:
        same(spec.decode_batch(H, y[snr], snr), gen.decode_batch(H, y[snr], snr), name, snr)
        # the state evolution is deterministic: frames frozen, sweeps not run, store and compare passes, to the unit
        sa, sb = spec.freeze_stats(H), gen.freeze_stats(H)
        pa, pb = spec.freeze_passes(H), gen.freeze_passes(H)
        print("%s %+.0f dB: frozen, sweeps not run %s / %s; store, compare passes %s / %s (spec / generic)" % (name, snr, sa, sb, pa, pb))
        assert sa == sb and pa == pb, (name, snr)
    for snr in (-2.0, 2.0):
        a = A.run_experiment(spec, cws, H, snr, frames=4096, noise="device", seed=15)
        b = A.run_experiment(gen, cws, H, snr, frames=4096, noise="device", seed=15)
        va, vb = [int(x) for x in a.as_vector()], [int(x) for x in b.as_vector()]
        assert len(va) == 7 and va == vb and a.total == 4096, (name, snr, va, vb)
    spec.close()
    gen.close()
