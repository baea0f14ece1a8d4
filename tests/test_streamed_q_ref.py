"""CPU: the sparse restatement of the streamed fixed-point layered min-sum engine (tests/streamed_q_ref.py) against the pinned
one (tests/layered_q_io_ref.decode_int): word, flag, iteration and every posterior of every frame equal — on the six cases of
tests/layered_q_cases.py for the three quantisers, and on two codes with checks of 48 and 40 variables, where decode_int runs
over single-check layers (its sets come from layers_wide(), which stops at 32)."""
import numpy as np
import pytest

import layered_q_cases as Q
import layered_q_io_cases as IO
import streamed_q_cases as S
from layered_q_io_ref import decode_int
from streamed_q_ref import decode_int_sparse, edges_of, single_check_layers


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def _same(got, want, ctx):
    for name, g, w in zip(("word", "flag", "iteration", "posterior"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, name)
        bad = g != w
        assert not bad.any(), "%s: %s differs in %d places, first at %s" % (ctx, name, int(bad.sum()), tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_sparse_equals_decode_int(A, name, qname):
    """the sets of layers_any() are those of layers_wide() where the latter accepts; 0 and 1 iterations too"""
    c = Q.case(A, name)
    Z, layers = c.H.layers_any()
    assert Z == c.Z and np.array_equal(layers, c.layers)
    ch = IO.channel(A, name, qname)
    edges = edges_of(c.Hm)
    _same(decode_int_sparse(edges, c.n, layers, ch, c.iters, Q.QUANTS[qname]), IO.ref(A, name, qname), (name, qname))
    for it in (0, 1):
        _same(decode_int_sparse(edges, c.n, layers, ch, it, Q.QUANTS[qname]), IO.ref(A, name, qname, it), (name, qname, it))
    # single-check layers in the order of the sets: the same results, since a set's checks share no variable
    singles = [[k] for layer in layers for k in layer if k >= 0]
    _same(decode_int_sparse(edges, c.n, singles, ch, c.iters, Q.QUANTS[qname]), IO.ref(A, name, qname), (name, qname, "singles"))


@pytest.mark.parametrize("name", ["deg48", "deg40"])
def test_sparse_equals_decode_int_on_wide_checks(A, name):
    """decode_int takes checks of 48 and 40 variables unchanged; its layers are single checks in the order of the sets of
    layers_any()"""
    w = S.wide(A, name)
    assert max(len(e) for e in w.edges) == S.WIDE[name][0][3] > 32
    singles = [[k] for layer in w.layers for k in layer if k >= 0]
    assert sorted(k for (k,) in singles) == list(range(w.m))
    Hm = np.zeros((w.m, w.n), dtype=np.uint8)
    for k, e in enumerate(w.edges):
        Hm[k, e] = 1
    for qname in sorted(Q.QUANTS):
        want = decode_int(Hm, singles, w.channel(qname), w.iters, Q.QUANTS[qname])
        _same(w.ref(qname), want, (name, qname))
        _same(decode_int_sparse(w.edges, w.n, single_check_layers(w.edges), w.channel(qname), w.iters, Q.QUANTS[qname]),
              decode_int(Hm, single_check_layers(w.edges), w.channel(qname), w.iters, Q.QUANTS[qname]), (name, qname, "row order"))
    ok = w.ref("default")[1]
    assert 0 < ok.sum() < w.frames, (name, int(ok.sum()))
