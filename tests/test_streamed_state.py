"""CPU: why the state of the streamed layered engines is compared word for word (tests/test_streamed_state_gpu.py) — a census,
on the `tails` case of tests/streamed_state_cases.py, of departures from the restatements that the three hard outputs of a
frame (word, flag, iteration count) do not show and its final posteriors and messages do.

Measured with layered_ref.host_phi on the 101 frames of the case (print lines of test_departures_change_the_state; -s shows
them).  Words of P (101 x 120 = 12 120) / of R (101 x 328 = 33 128) that differ after 2 and after 25 iterations, and frames of
101 with another word, flag or count after 1, 2, 3, 10 or 25 iterations (the five runs added up):

  departure                                              rule      P 2 / 25       R 2 / 25        hard outputs
  edges rotated by one                                   bp        3490 / 7021    17653 / 23758   0
  suffix accumulated ascending                           bp        3303 / 7023    16448 / 23466   0
  prefix from +0 inside each chunk of 8, base added      bp        1733 / 6386     9558 / 20917   0
  P' = p + (r' - r) instead of P' = q + r'               bp        5218 / 8191     8201 / 21186   0
  the same                                               minsum    5087 / 8418     5827 / 19321   0

  latched frames written too, after 10 iterations, words of the frames that latched before:
                                                         bp        6480 of 6480   17658 of 17712  0      (54 frames)
                                                         minsum    6152 of 6720   15526 of 18368  0      (56 frames)

So none of them is visible to a test of the hard outputs on these frames, and each moves thousands of state words.  The fourth
equals the rule in the first iteration (r = 0 there), so no frame of one iteration can see it either.  (A rotated check's
messages are put back into ascending order before they are compared: the words counted differ in value, not in place.)"""
import ctypes as C

import numpy as np
import pytest

import streamed_state_cases as SS
from layered_ref import LOG2E_F32, SPA_SATURATION, _run_layered, channel_llr_f32, host_phi, layered_sumproduct_exact, spa_messages

ITERS = 25
DEPARTURES = {
    # name: (rules it applies to, how it is made)
    "rotate_edges": (("bp",), "variant"),
    "suffix_ascending": (("bp",), "variant"),
    "chunk_prefix": (("bp",), "local"),
    "p_plus_delta": (("bp", "minsum"), "local"),
}


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


@pytest.fixture(scope="module")
def c(A):
    return SS.tails(A)


def _spa_chunk_prefix(q, phi):
    """spa_messages with ONE departure: the prefix of edge j is summed from +0 inside j's chunk of 8 edges and the ascending sum
    at the start of the chunk is added afterwards, pre_j = base_c + (mag_8c + ... + mag_{j-1}), where the rule is the one
    ascending sum ((base_c + mag_8c) + ...) + mag_{j-1}.  The same for a check of up to 8 edges."""
    D = q.shape[-1]
    mag = phi(np.abs(q))
    pre, suf = np.empty_like(mag), np.empty_like(mag)
    total = np.zeros(mag.shape[:-1], dtype=np.float32)
    for j in range(D):
        if j % 8 == 0:
            base, local = total, np.zeros(mag.shape[:-1], dtype=np.float32)
        pre[..., j] = base + local
        local = local + mag[..., j]
        total = total + mag[..., j]
    s = np.zeros(mag.shape[:-1], dtype=np.float32)
    for j in range(D - 1, -1, -1):
        suf[..., j] = s
        s = s + mag[..., j]
    out = np.fmin(phi(pre + suf), SPA_SATURATION)
    assert out.dtype == np.float32
    sq = np.signbit(q)
    neg = np.logical_xor.reduce(sq, axis=-1)[..., None] ^ sq
    return np.where(neg, -np.abs(out), np.abs(out)).astype(np.float32)


def _minsum_messages(q, scale):
    """the check rule of layered_ref.layered_minsum (fp32 messages) on q [F, D]"""
    F, D = q.shape
    a = np.abs(q)
    srt = np.sort(a, axis=1)
    m1, m2 = srt[:, 0], (srt[:, 1] if D > 1 else np.full(F, np.inf, np.float32))
    m1s = (np.float64(scale) * m1.astype(np.float64)).astype(np.float32)
    with np.errstate(over="ignore"):
        m2s = (np.float64(scale) * m2.astype(np.float64)).astype(np.float32)
    if D == 1:
        m2s = np.full(F, np.float32(59968.0), dtype=np.float32)
    mag = np.where(a == m1[:, None], m2s[:, None], m1s[:, None]).astype(np.float32)
    sq = np.signbit(q)
    neg = np.logical_xor.reduce(sq, axis=1)[:, None] ^ sq
    return np.where(neg, -mag, mag).astype(np.float32)


def _local(c, algo, it, departure=None):
    """a check-by-check restatement over the control skeleton of layered_ref (_run_layered), test-local so that it can depart:
    None            the rule (held to layered_minsum / layered_sumproduct_exact bit for bit by test_local_restatement_is_the_rule)
    "chunk_prefix"  _spa_chunk_prefix for spa_messages
    "p_plus_delta"  P' = p + (r' - r) for P' = q + r'
    "latched_write" P and R are written for latched frames too (their word, flag and count were taken when they latched)
    -> (bits, ok, iters, P [F, n], R [F, E] in processing order)"""
    F = c.frames
    P = channel_llr_f32(c.y, c.snr)
    if algo == "bp":
        P = P * LOG2E_F32
    R = {k: np.zeros((F, len(c.edges[k])), dtype=np.float32) for k in c.order}

    def layer_step(li, ids, live):
        loud = np.zeros(F, dtype=bool)
        for k in ids:
            v, r = c.edges[k], R[k]
            p = P[:, v]
            q = p - r
            if algo == "minsum":
                rn = _minsum_messages(q, np.float32(SS.MS_SCALE))
            else:
                rn = _spa_chunk_prefix(q, host_phi) if departure == "chunk_prefix" else spa_messages(q, host_phi)
            pn = p + (rn - r) if departure == "p_plus_delta" else q + rn
            assert pn.dtype == np.float32
            loud |= np.logical_xor.reduce(np.signbit(p), axis=1) | (np.signbit(pn) != np.signbit(p)).any(axis=1)
            w = np.ones(F, dtype=bool) if departure == "latched_write" else live
            P[np.ix_(w, v)] = pn[w]
            R[k][w] = rn[w]
        return loud
    res = _run_layered(c.Hm, c.layers, P, it, layer_step)
    return tuple(res) + (P, np.concatenate([R[k] for k in c.order], axis=1))


def _departed(c, algo, it, name):
    if DEPARTURES.get(name, (None, "local"))[1] == "local":
        return _local(c, algo, it, name)
    P, R = [], []
    res = layered_sumproduct_exact(c.Hm, c.layers, c.y, c.snr, it, host_phi, variant=name, posteriors=P, messages=R)
    if name == "rotate_edges":            # its messages come in ITS edge order, each check's last variable first: back to ascending
        cols, e0 = [], 0
        for k in c.order:
            D = len(c.edges[k])
            cols += list(e0 + np.roll(np.arange(D), -1))
            e0 += D
        R = [R[0][:, cols]]
    return tuple(res) + (P[0], R[0])


def _words(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _hard(a, b):
    return int(((a[0] != b[0]).any(axis=1) | (a[1] != b[1]) | (a[2] != b[2])).sum())


def test_the_graph_has_every_tail():
    Hm = SS.matrix()
    deg = Hm.sum(axis=1)
    assert Hm.shape == (23, 120) and sorted(int(d) for d in deg) == SS.TAILS_DEGREES and int(deg.sum()) == 328
    wide = [int(d) for d in deg if d > 8]
    assert {d % 8 for d in wide} == set(range(8))
    for tail in range(1, 8):
        assert any(d % 8 == tail for d in wide), tail
    for d in (13, 14, 21, 22, 29, 30):          # tails 5 and 6 behind one, two and three full chunks
        assert d in wide
    used = Hm.sum(axis=0)
    assert (used > 0).all() and (used >= 2).mean() > 0.75, used


def test_sets_are_single_checks_in_the_library_order(c):
    """one degree per set and every degree once: 23 sets of one check each; edge_var is the engines' CSR"""
    assert c.Z == 0 and len(c.order) == 23 and sorted(c.order) == list(range(23)) and c.E == 328
    assert all((layer >= 0).sum() == 1 for layer in c.layers)
    assert c.edge_var.shape == (328,) and all((np.diff(c.edges[k]) > 0).all() for k in c.order)


@pytest.mark.parametrize("algo", SS.ALGOS)
def test_restatement_latches_some_frames_and_fails_others_in_both_tiles(c, algo):
    ref = c.ref(algo, ITERS)
    ok, iters = ref[1], ref[2]
    print("%s at %.1f dB: %d of %d decoded, exit iterations %s" % (algo, c.snr, int(ok.sum()), c.frames, sorted(set(iters[ok == 1].tolist()))))
    assert 0 < ok.sum() < c.frames
    assert (iters[ok == 1] < 3).any() and (iters[ok == 1] > 3).any()
    for tile in (slice(0, 64), slice(64, 101)):
        assert 0 < ok[tile].sum() < len(ok[tile]) and (iters[tile][ok[tile] == 1] < ITERS).any()
    assert not np.isnan(ref[3]).any() and not np.isnan(ref[4]).any()


@pytest.mark.parametrize("algo", SS.ALGOS)
def test_local_restatement_is_the_rule(c, algo):
    """the test-local restatement without a departure has every bit of the committed one's answers and state"""
    for it in (2, ITERS):
        want, got = c.ref(algo, it), _local(c, algo, it)
        assert _hard(got, want) == 0 and _words(got[3], want[3]) == 0 and _words(got[4], want[4]) == 0, (algo, it)


@pytest.mark.parametrize("name", sorted(DEPARTURES))
def test_departures_change_the_state(c, name):
    """each one-line departure changes posterior AND message words after 2 iterations; how many, and how many hard outputs, is
    printed (the module's docstring and DESIGN 3i carry the figures).  That the hard outputs stay equal is the observation this
    module records, not a requirement: nothing here asserts it."""
    for algo in DEPARTURES[name][0]:
        hard = 0
        for it in (1, 2, 3, 10, ITERS):
            want, got = c.ref(algo, it), _departed(c, algo, it, name)
            hard += _hard(got, want)
            if it in (2, ITERS):
                dp, dr = _words(got[3], want[3]), _words(got[4], want[4])
                print("%s %s after %d iterations: %d of %d posterior words, %d of %d message words differ"
                      % (name, algo, it, dp, want[3].size, dr, want[4].size))
                if it == 2:
                    assert dp > 0 and dr > 0, (name, algo, dp, dr)
        print("%s %s: %d hard outputs differ over 1, 2, 3, 10 and %d iterations" % (name, algo, hard, ITERS))


@pytest.mark.parametrize("algo", SS.ALGOS)
def test_writing_latched_frames_changes_their_state(c, algo):
    """the rule: a latched frame computes on but writes nothing.  A restatement that goes on writing changes the state of the
    frames that latched before iteration 10, and of no other frame"""
    want, got = c.ref(algo, 10), _local(c, algo, 10, "latched_write")
    latched = (want[1] == 1) & (want[2] < 10)
    assert latched.any() and not latched.all()
    dp, dr = _words(got[3][latched], want[3][latched]), _words(got[4][latched], want[4][latched])
    print("latched_write %s after 10 iterations: %d of %d posterior words, %d of %d message words of the %d latched frames differ; "
          "%d hard outputs" % (algo, dp, want[3][latched].size, dr, want[4][latched].size, int(latched.sum()), _hard(got, want)))
    assert dp > 0 and dr > 0
    assert (got[3][latched].view(np.uint32) != want[3][latched].view(np.uint32)).any(axis=1).all()      # every latched frame
    assert _words(got[3][~latched], want[3][~latched]) == 0 and _words(got[4][~latched], want[4][~latched]) == 0


def test_state_requests_leave_the_answers_alone(c):
    """posteriors= / messages= only hand out what the restatements hold: the answers with and without them are equal"""
    from layered_ref import layered_minsum
    plain = layered_minsum(c.Hm, c.layers, c.y, c.snr, 3, SS.MS_SCALE)
    assert _hard(plain, c.ref("minsum", 3)) == 0
    plain = layered_sumproduct_exact(c.Hm, c.layers, c.y, c.snr, 3, host_phi)
    assert _hard(plain, c.ref("bp", 3)) == 0
    q = c.qref("default", 3)
    assert q[4].dtype == np.int8 and q[4].shape == (c.frames, c.E) and q[3].dtype == np.int16 and q[4].any()


def test_debug_entry_is_declared_and_refuses_a_null_handle(A):
    L = A.lib()
    name = "acg_ldpc_debug_streamed_slab"
    assert name in A._lib.SYMBOLS and getattr(L, name).restype is C.c_int
    size = C.c_int64(-1)
    rc = L.acg_ldpc_debug_streamed_slab(None, 0, None, 0, C.byref(size))
    assert rc != 0 and "null decoder" in L.acg_ldpc_last_error().decode() and size.value == 0
    rc = L.acg_ldpc_debug_streamed_slab(None, 0, None, 0, None)
    assert rc != 0 and "null slab_bytes" in L.acg_ldpc_last_error().decode()
