"""Build-time instances of the fused fixed-work sum-product kernel with a code's pass structure constant (bp_inst_spec.hip, static
pass policy of bp_core.inc): only values that are the same for every lane become constants, so every output and every device
counter equals that of the generic instance, which a handle created under ACG_BP_NO_SPEC=1 keeps.  The switch is read when a
handle is created; both handles live in this process.  One case per entry of the default SPEC_CODES (csrc/Makefile): the code is
the smallest shape an instance exists for, so the batches are small instead.  Run with `-m gpu` on an MI355X."""
import contextlib
import os

import numpy as np
import pytest

import acg_alp_ldpc_amd as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"H05_L32": ("H05", 32, 64), "H_L64": ("H", 64, 32), "optimalH_L32": ("optimalH", 32, 64)}  # name: matrix, its width, another
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


def decoder(H, generic, max_iter=50, **kw):
    """(decoder, describe()) with its handle for H created with or without the switch"""
    d = A.BeliefPropagationDecoder(max_iter, **{"early_exit": False, **kw})
    with no_spec(generic):
        text = d.describe(H)
    return d, text


@pytest.fixture(scope="module", params=sorted(ENTRIES))
def entry(request):
    """per entry: name, H, codewords and per SNR the symbols of the largest batch, made once and left alone"""
    from oracle.pyoracle import Oracle
    name = request.param
    matrix, L, other = ENTRIES[name]
    H = A.ParityCheckMatrix(Oracle().read_pcm(os.path.join(ROOT, "data", matrix + ".txt")))
    G, ok = H.get_orthogonal()
    assert ok
    cws = A.gen_random_codewords(G, 64, 1414)
    y = {snr: A.transmit_frames(cws[np.arange(max(FRAMES)) % len(cws)], snr) for snr in SNRS}
    return name, L, other, H, cws, y


def test_selection(entry):
    name, L, other, H, _, _ = entry
    cases = [(dict(), False, "spec=" + name), (dict(), True, "spec=0"), (dict(early_exit=True), False, "spec=0"),
             (dict(lanes_per_frame=other), False, "spec=0"), (dict(lanes_per_frame=L), False, "spec=" + name)]
    for kw, generic, want in cases:
        d, text = decoder(H, generic, **kw)
        assert text.endswith(" " + want), (kw, generic, text)
        assert "kernel=bp_fused_kernel" in text and ("lanes_per_frame=%d " % kw.get("lanes_per_frame", L)) in text, text
        d.close()


def test_outputs_and_freeze_counters_equal(entry):
    name, L, _, H, _, y = entry
    for max_iter in MAX_ITERS:
        spec, t_spec = decoder(H, False, max_iter)
        gen, t_gen = decoder(H, True, max_iter)
        assert t_spec.endswith(" spec=" + name) and t_gen.endswith(" spec=0"), (t_spec, t_gen)
        assert spec.freeze_stats(H) == (0, 0) and gen.freeze_stats(H) == (0, 0)   # counting on from here
        for snr in SNRS:
            for frames in FRAMES:
                a, b = spec.decode_batch(H, y[snr][:frames], snr), gen.decode_batch(H, y[snr][:frames], snr)
                for k, what in enumerate(("bits", "ok", "iters")):
                    assert np.array_equal(a[k], b[k]), (name, max_iter, snr, frames, what, int((a[k] != b[k]).sum()))
                if frames == max(FRAMES):
                    # the state evolution is deterministic: frames frozen, sweeps not run, store and compare passes, to the unit
                    sa, sb = spec.freeze_stats(H), gen.freeze_stats(H)
                    pa, pb = spec.freeze_passes(H), gen.freeze_passes(H)
                    print("%s max_iter=%d %+.0f dB: frozen, sweeps not run %s / %s; store, compare passes %s / %s (spec / generic)"
                          % (name, max_iter, snr, sa, sb, pa, pb))
                    assert sa == sb and pa == pb, (name, max_iter, snr)
                    if name == "H05_L32" and max_iter == 50 and snr == 2.0:
                        assert sa[0] > 0 and pa[0] > 0, "the freeze path ran"
                else:
                    spec.freeze_stats(H), gen.freeze_stats(H), spec.freeze_passes(H), gen.freeze_passes(H)
        spec.close()
        gen.close()


def test_monte_carlo_counters_equal(entry):
    name, _, _, H, cws, _ = entry
    spec, t_spec = decoder(H, False)
    gen, t_gen = decoder(H, True)
    assert t_spec.endswith(" spec=" + name) and t_gen.endswith(" spec=0"), (t_spec, t_gen)
    for snr in (-2.0, 2.0):
        a = A.run_experiment(spec, cws, H, snr, frames=4096, noise="device", seed=14)
        b = A.run_experiment(gen, cws, H, snr, frames=4096, noise="device", seed=14)
        va, vb = [int(x) for x in a.as_vector()], [int(x) for x in b.as_vector()]
        assert len(va) == 7 and va == vb and a.total == 4096, (name, snr, va, vb)
    spec.close()
    gen.close()
