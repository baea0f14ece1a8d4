"""GPU: acg_ldpc_mc_run_detail against an expectation the code under test never computes: the symbols of
acg_ldpc_awgn_dev (device noise) or acg_ldpc_transmit_host (host noise), decoded through decode_batch_dev / decode_batch on
the same decoder parameters, classified by the numpy restatement tests/mc_detail_ref.py.  Every field of the struct except
the two times, every event and every bit of the XOR rows must be equal."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mc_detail_ref as R  # noqa: E402
from mc_decode_path import decode_device_noise, sent_words  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 1000                 # with ACG_MC_DETAIL_CHUNK=300: four chunks, the last one partial, none a multiple of 64
FIRST = (1 << 33) + 5         # the high half of the global frame index matters
NCW = 7                       # codewords cycle with a period that divides nothing


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    A.build()
    return A


@pytest.fixture(scope="module")
def codes(A):
    """name -> (ParityCheckMatrix, dense H, 7 codewords)"""
    out = {}
    for name, H in (("H", A.read_pcm(os.path.join(DATA, "H.txt"))), ("H05", A.read_pcm(os.path.join(DATA, "H05.txt"))),
                    ("reg40", A.ParityCheckMatrix(A.regular_ldpc(20, 40, 3, 6)))):
        G, ok = H.get_orthogonal()
        assert ok
        out[name] = (H, H.dense(), A.gen_random_codewords(G, NCW, 2024))
    return out


def chunked(value):
    if value is None:
        os.environ.pop("ACG_MC_DETAIL_CHUNK", None)
    else:
        os.environ["ACG_MC_DETAIL_CHUNK"] = str(value)


@pytest.fixture(autouse=True)
def _chunk_env():
    chunked(300)
    yield
    chunked(None)


def expectation(A, dec, H, Hd, cws, snr, frames, first, seed, noise, cap):
    sent = sent_words(cws, H.n, first, frames)
    if noise == "device":
        y, words, ok, it = decode_device_noise(A, dec, H, cws, snr, frames, first, seed)
    else:
        y = A.transmit_frames(cws if cws is not None else np.zeros((1, H.n), np.uint8), snr, first_frame=first, frames=frames)
        bits, ok, it = dec.decode_batch(H, y, snr) if frames else (np.zeros((0, H.n), np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.int32))
        words = R.pack_bits(bits) if frames else np.zeros((0, (H.n + 31) // 32), np.uint32)
    return R.mc_detail(y, words, ok, it, sent, Hd, first_frame=first, cap=cap)


def counters(d):
    return {f: getattr(d, f) for f in R.COUNTERS}


def assert_equal(d, exp, words=True, what=""):
    c, ev, rows = exp
    assert counters(d) == c, what
    assert d.events.dtype == ev.dtype and (d.events == ev).all(), what
    if words:
        assert d.words.dtype == np.uint32 and d.words.shape == rows.shape and (d.words == rows).all(), what
    else:
        assert d.words is None


def cut(exp, cap):
    """the expectation of the same run with a smaller cap"""
    c, ev, rows = exp
    c = dict(c, n_stored=min(cap, len(ev)))
    return c, ev[:cap], rows[:cap]


def decoders(A):
    """name -> (constructor, code, snr, seed, kinds that must occur).  SNR and seed were chosen so that the coverage condition
    holds (H05 at -2 dB: 915 correct and 4 pseudo of 1000 for BP-50, tests/golden/known_answers.json)."""
    L = A.SCHEDULE_LAYERED
    P, N, X = R.EVENT_PSEUDO, R.EVENT_NO_WORD, R.EVENT_NONCODEWORD
    return {
        "bp_flood": (lambda: A.BeliefPropagationDecoder(50), "H05", -2.0, 2, {P, N}),
        "bp_flood_fixed_work": (lambda: A.BeliefPropagationDecoder(50, early_exit=False), "H05", -2.0, 2, {P, N}),
        "ms_flood": (lambda: A.MinSumDecoder(50, 0.75), "H05", -2.0, 2, {P, N}),
        "ms_pair_f16": (lambda: A.MinSumDecoder(50, 0.75, precision=A.PREC_F16), "reg40", 0.0, 1, {P, N}),   # (the pair kernel needs variable degree <= 4)
        "ms_layered_f32": (lambda: A.MinSumDecoder(25, 0.75, schedule=L), "H05", -2.0, 2, {P, N}),
        "ms_layered_f16": (lambda: A.MinSumDecoder(25, 0.75, schedule=L, precision=A.PREC_F16), "H05", -2.0, 2, {P, N}),
        "ms_layered_block256": (lambda: A.MinSumDecoder(25, 0.75, schedule=L, lanes_per_frame=256), "H05", -2.0, 2, {P, N}),
        "bp_streamed": (lambda: A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED), "H05", -2.0, 2, {P, N}),
        "admm_lds": (lambda: A.QPADMMDecoder(1.95, 0.5, 100, fast_setup=True), "H05", -2.0, 2, {X}),
        "admm_streamed": (lambda: A.QPADMMDecoder(1.95, 0.5, 100, engine=A.ENGINE_STREAMED), "H05", -2.0, 2, {X}),
        "bp_flood_H128": (lambda: A.BeliefPropagationDecoder(50), "H", -2.0, 2, {P, N}),
        "bp_flood_n40": (lambda: A.BeliefPropagationDecoder(50), "reg40", 0.0, 1, {P, N}),
        "admm_lds_n40": (lambda: A.QPADMMDecoder(1.95, 0.5, 100, fast_setup=True), "reg40", 0.0, 1, {X}),
    }


CASES = ["bp_flood", "bp_flood_fixed_work", "ms_flood", "ms_pair_f16", "ms_layered_f32", "ms_layered_f16", "ms_layered_block256",
         "bp_streamed", "admm_lds", "admm_streamed", "bp_flood_H128", "bp_flood_n40", "admm_lds_n40"]


def replay(A, dec, H, cws, snr, seed, d, limit=8):
    """a stored event's frame index alone reproduces it: generate that one global frame, decode it, compare"""
    for k in range(min(limit, d.n_stored)):
        e = d.events[k]
        y, words, ok, it = decode_device_noise(A, dec, H, cws, snr, 1, int(e["frame"]), seed)
        sent = R.pack_bits(sent_words(cws, H.n, int(e["frame"]), 1))
        assert bool(ok[0]) == (int(e["kind"]) != R.EVENT_NO_WORD), k
        assert int(it[0]) == int(e["iters"]), k
        want = (words[0] ^ sent[0]) if ok[0] else np.zeros_like(sent[0])
        assert (d.words[k] == want).all(), k


@pytest.mark.parametrize("name", CASES)
def test_detail_matches_decode_path(A, codes, name):
    make, code, snr, seed, kinds = decoders(A)[name]
    H, Hd, cws = codes[code]
    dec = make()
    exp = expectation(A, dec, H, Hd, cws, snr, FRAMES, FIRST, seed, "device", cap=FRAMES)
    n_events = exp[0]["n_events"]
    print(name, exp[0], np.bincount(exp[1]["kind"], minlength=4).tolist())
    run = lambda **kw: A.run_experiment_detail(dec, cws, H, snr, frames=FRAMES, first_frame=FIRST, noise="device", seed=seed, **kw)  # noqa: E731
    full = run(cap=FRAMES, words=True)
    assert_equal(full, exp, what="cap above n_events, words")
    # coverage: the case really holds what it claims to cover
    assert kinds <= set(full.events["kind"].tolist()), (kinds, np.bincount(full.events["kind"], minlength=4))
    assert 0 < n_events < FRAMES
    # cap 0 / 3 / above n_events, with and without words
    assert_equal(run(cap=0), cut(exp, 0), words=False, what="cap 0")
    assert_equal(run(cap=0, words=True), cut(exp, 0), what="cap 0, words")
    three = run(cap=3, words=True)
    assert_equal(three, cut(exp, 3), what="cap 3")
    assert three.events["frame"].tolist() == sorted(exp[1]["frame"].tolist())[:3]      # the three lowest frames
    assert_equal(run(cap=3), cut(exp, 3), words=False, what="cap 3, no words")
    assert_equal(run(cap=n_events + 9), exp, words=False, what="cap above n_events")
    # determinism over the chunking
    for chunk in (64, None):
        chunked(chunk)
        assert_equal(run(cap=FRAMES, words=True), exp, what="chunk %s" % chunk)
        assert_equal(run(cap=3, words=True), cut(exp, 3), what="chunk %s cap 3" % chunk)
    chunked(300)
    # two shards, merged
    for cap in (3, FRAMES):
        a = A.run_experiment_detail(dec, cws, H, snr, frames=417, first_frame=FIRST, noise="device", seed=seed, cap=cap, words=True)
        b = A.run_experiment_detail(dec, cws, H, snr, frames=FRAMES - 417, first_frame=FIRST + 417, noise="device", seed=seed, cap=cap, words=True)
        assert_equal(A.merge_exp_details(b, a), cut(exp, cap), what="shards, cap %d" % cap)
    replay(A, dec, H, cws, snr, seed, full)
    # base against acg_ldpc_mc_run on the same cfg (for several engines that is a fused Monte-Carlo kernel)
    r = A.run_experiment(dec, cws, H, snr, frames=FRAMES, first_frame=FIRST, noise="device", seed=seed)
    assert {f: getattr(r, f) for f in r.FIELDS} == {f: getattr(full, f) for f in r.FIELDS}
    dec.close()


def test_guard_decoder_every_frame_is_no_word(A, codes):
    """e_min * mu <= alpha (qp_admm.h:108-114): no word is returned for any frame; acg_ldpc_mc_run refuses such a decoder with
    device noise on the LDS engine, the detail run reports the frames"""
    H, Hd, cws = codes["H05"]
    dec = A.QPADMMDecoder(100.0, 0.01, 100, fast_setup=True)
    exp = expectation(A, dec, H, Hd, cws, -2.0, FRAMES, FIRST, 3, "device", cap=FRAMES)
    d = A.run_experiment_detail(dec, cws, H, -2.0, frames=FRAMES, first_frame=FIRST, noise="device", seed=3, cap=FRAMES, words=True)
    assert_equal(d, exp)
    assert d.n_events == FRAMES and (d.events["kind"] == R.EVENT_NO_WORD).all() and not d.words.any()
    assert (d.word_frames, d.bit_errors, d.correct, d.pseudo, d.sum_iters, d.min_pseudo_weight) == (0, 0, 0, 0, 0, -1)
    assert d.sum_hamming == d.sum_hamming_wrong > 0
    assert_equal(A.run_experiment_detail(dec, cws, H, -2.0, frames=FRAMES, first_frame=FIRST, noise="device", seed=3, cap=3), cut(exp, 3), words=False)
    # host noise: acg_ldpc_mc_run accepts the decoder, same seven counters
    dh = A.run_experiment_detail(dec, cws, H, -2.0, frames=200, first_frame=FIRST, noise="host", cap=5)
    r = A.run_experiment(dec, cws, H, -2.0, frames=200, first_frame=FIRST, noise="host")
    assert {f: getattr(r, f) for f in r.FIELDS} == {f: getattr(dh, f) for f in r.FIELDS}
    assert dh.n_events == 200 and dh.n_stored == 5
    with pytest.raises(A.LdpcError, match="guard"):
        A.run_experiment(dec, cws, H, -2.0, frames=FRAMES, first_frame=FIRST, noise="device", seed=3)
    dec.close()


@pytest.mark.parametrize("name", ["bp_flood", "admm_lds"])
@pytest.mark.parametrize("noise,null_cw", [("host", False), ("host", True), ("device", True)])
def test_host_noise_and_null_codewords(A, codes, name, noise, null_cw):
    make, code, snr, seed, kinds = decoders(A)[name]
    H, Hd, cws = codes[code]
    cws = None if null_cw else cws
    dec = make()
    frames = 400 if noise == "host" else FRAMES
    exp = expectation(A, dec, H, Hd, cws, snr, frames, FIRST, seed, noise, cap=frames)
    run = lambda **kw: A.run_experiment_detail(dec, cws, H, snr, frames=frames, first_frame=FIRST, noise=noise, seed=seed, **kw)  # noqa: E731
    full = run(cap=frames, words=True)
    assert_equal(full, exp)
    assert 0 < full.n_events < frames and (kinds & set(full.events["kind"].tolist()))
    assert_equal(run(cap=3), cut(exp, 3), words=False)
    assert_equal(run(cap=0), cut(exp, 0), words=False)
    chunked(64)
    assert_equal(run(cap=frames, words=True), exp, what="chunk 64")
    r = A.run_experiment(dec, cws, H, snr, frames=frames, first_frame=FIRST, noise=noise, seed=seed)
    assert {f: getattr(r, f) for f in r.FIELDS} == {f: getattr(full, f) for f in r.FIELDS}
    dec.close()


@pytest.mark.parametrize("noise", ["host", "device"])
def test_zero_frames(A, codes, noise):
    H, Hd, cws = codes["H05"]
    dec = A.BeliefPropagationDecoder(50)
    for cap, words in ((0, False), (4, True)):
        d = A.run_experiment_detail(dec, cws, H, -2.0, frames=0, first_frame=FIRST, noise=noise, cap=cap, words=words)
        assert counters(d) == dict({f: 0 for f in R.COUNTERS}, min_pseudo_weight=-1, min_pseudo_frame=-1)
        assert len(d.events) == 0 and (d.words is None or d.words.shape == (0, 9))
    dec.close()
