"""CPU: the inputs of tests/test_cascade_shapes_gpu.py are what that module takes them for.  The code H05m1 has the row lengths
that keep cascade_gather_launch off its uint4 instance; the designed failure masks put failures on the tile boundaries of the
select scan; and the restatement (tests/layered_ref.py::layered_minsum on the library's own layering) fails EXACTLY the masked
frames in one iteration, and in 20 iterations decodes more than half and fewer than all of them, each to its own word — so the
merged output the GPU tests expect contains none of the code under test and shows a mis-scattered row."""
import numpy as np
import pytest

import cascade_shapes_cases as S
import layered_q_cases as Q
from layered_q_io_ref import decode_int
from layered_q_ref import quantize
from mc_detail_ref import unpack_bits


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def test_code_has_no_16_byte_rows(A):
    c = S.code(A)
    assert (c.m, c.n) == (160, 279) and S.gf2_rank(c.Hm) == 160
    assert [(c.n * e) % 16 for e in (4, 8, 2)] == [12, 8, 14]
    assert c.Z == 0, "H05 without a column is not quasi-cyclic"
    ids = c.layers[c.layers >= 0]
    assert sorted(ids) == list(range(c.m))
    for layer in c.layers:
        assert (c.Hm[layer[layer >= 0]].sum(axis=0) <= 1).all()
    assert len(np.unique(c.cws, axis=0)) == S.NCW


def test_masks_sit_on_the_tile_boundaries():
    t = S.tile_masks().reshape(5, 2 * S.TILE)
    assert list(np.flatnonzero(t[0])) == [1023] and list(np.flatnonzero(t[1])) == [1024, 2047]
    assert not t[2, :1024].any() and t[2, 1024:].all()
    assert list(np.flatnonzero(t[3])[:4]) == [0, 63, 64, 127] and t[3].sum() == 64
    assert 900 < t[4].sum() < 1150 and t[4, :1024].any() and t[4, 1024:].any()
    o = S.odd_mask()
    assert len(o) == 2051 and o[[1024, 1025, 2050]].all() and 500 < o.sum() < 750


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["tiles", "odd"])
def test_stage_0_fails_exactly_the_masked_frames(A, name, dtype):
    c = S.code(A)
    fail, y, r = S.restated(A, name, dtype)
    F = len(fail)
    assert (r.ok0 == ~fail).all(), "noisy frames that pass one iteration: %s; clean frames that fail it: %s" % (
        np.flatnonzero(fail & (r.ok0 == 1))[:8], np.flatnonzero(~fail & (r.ok0 == 0))[:8])
    sent = S.sent(c, F, S.masks()[name][1])
    assert (r.it0[~fail] == 1).all() and (r.bits0[~fail] == sent[~fail]).all()
    # stage 1: more than half and fewer than all of the failed frames, and those to the word that was sent
    K = int(fail.sum())
    assert len(r.ok1) == K and K / 2 < r.ok1.sum() < K, (K, int(r.ok1.sum()))
    words, ok, it, stage = r.out
    assert (stage == np.where(fail, 2, 1)).all()
    good = fail & (ok == 1)
    assert (unpack_bits(words, c.n)[good] == sent[good]).mean() > 0.999
    assert (words[good][1:] != words[good][:-1]).any(axis=1).all()        # a row scattered one place off is another word
    assert len(np.unique(it[good])) > 5


def test_quantized_stage_0_fails_exactly_the_masked_frames(A):
    """the int16 hand-over test runs a one-iteration fixed-point first stage on 1100 frames: the design holds for it too"""
    c = S.code(A)
    fail, first = S.q_mask()
    y = S.symbols(A, c, fail, first)
    quant = Q.QUANTS["default"]
    Z, layers = c.H.layers_wide()
    ok = decode_int(c.Hm, layers, quantize(y, S.SNR, quant), 1, quant)[1]
    assert (ok == ~fail).all()
