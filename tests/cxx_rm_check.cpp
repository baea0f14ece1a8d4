// Compiled and, on a GPU box, run by tests/test_rm_gpu.py (tests/test_rm_cabi.py compiles it and runs it without a device):
// run_rate_matched of acg_ldpc::StreamedLayeredMinSumDecoder / QuantizedMinSumDecoder / StreamedQuantizedMinSumDecoder of
// include/acg_ldpc_decoder.hpp must compile with plain g++ against include/ and return the seven counters of acg_ldpc_mc_run_rm
// on the class's own handle, for a pattern and for none.
#include <cstdio>
#include <cstring>

#include "acg_ldpc_decoder.hpp"

using namespace acg_ldpc;

static bool same(const acg_ldpc_mc_result &a, const acg_ldpc_mc_result &b) {
    return a.correct == b.correct && a.pseudo == b.pseudo && a.total == b.total && a.sum_hamming == b.sum_hamming &&
           a.sum_hamming_ok == b.sum_hamming_ok && a.sum_hamming_wrong == b.sum_hamming_wrong && a.sum_iters == b.sum_iters;
}

template <class Dec>
static int run(Dec &dec, const TMatrix &H, const acg_ldpc_mc_cfg &cfg, const std::vector<uint8_t> &pattern) {
    const acg_ldpc_mc_result a = dec.run_rate_matched(H, cfg, pattern), none = dec.run_rate_matched(H, cfg);
    acg_ldpc_mc_result b, bn;
    if (acg_ldpc_mc_run_rm(dec.handle(H), &cfg, pattern.data(), &b) || acg_ldpc_mc_run_rm(dec.handle(H), &cfg, nullptr, &bn)) {
        std::fprintf(stderr, "%s\n", acg_ldpc_last_error());
        return 1;
    }
    const int ok = same(a, b) && same(none, bn) && a.total == cfg.frames && a.sum_hamming < none.sum_hamming;
    std::printf("%s frames=%lld same=%d correct=%lld,%lld raw=%lld,%lld\n", dec.name().c_str(), (long long) a.total, ok, (long long) a.correct,
                (long long) none.correct, (long long) a.sum_hamming, (long long) none.sum_hamming);
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    acg_ldpc_code *code = nullptr;
    if (acg_ldpc_code_load_txt(argv[1], &code)) {
        std::fprintf(stderr, "%s\n", acg_ldpc_last_error());
        return 3;
    }
    int m, n, E;
    acg_ldpc_code_dims(code, &m, &n, &E);
    std::vector<uint8_t> dense((size_t) m * n);
    acg_ldpc_code_dense(code, dense.data());
    TMatrix H(m, TCodeword(n));
    for (int i = 0; i < m; i++)
        for (int j = 0; j < n; j++) H[i][j] = dense[(size_t) i * n + j];
    acg_ldpc_mc_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.frames = 200;
    cfg.first_frame = 11;
    cfg.snr = -2.0;
    cfg.seed = 7;
    cfg.noise = ACG_LDPC_NOISE_DEVICE_PHILOX;
    acg_ldpc_mc_result r;
    const int rc = acg_ldpc_mc_run_rm(nullptr, &cfg, nullptr, &r);
    std::printf("n=%d null handle: %s\n", n, rc ? acg_ldpc_last_error() : "accepted");
    if (rc == 0) return 4;
    StreamedLayeredMinSumDecoder ms(15, 0.75);
    QuantizedMinSumDecoder q(15);
    StreamedQuantizedMinSumDecoder qs(15);
    if (!acg_ldpc_device_available()) {
        std::printf("no device: compile/link check only\n");
        return 0;
    }
    std::vector<uint8_t> pattern((size_t) n, (uint8_t) ACG_LDPC_RM_SENT);   // the all-zero word: every tenth position punctured or shortened
    for (int v = 0; v < n; v++) pattern[(size_t) v] = (uint8_t) (v % 20 == 3 ? ACG_LDPC_RM_PUNCTURED : v % 20 == 11 ? ACG_LDPC_RM_SHORTENED : ACG_LDPC_RM_SENT);
    const int bad = run(ms, H, cfg, pattern) + run(q, H, cfg, pattern) + run(qs, H, cfg, pattern);
    acg_ldpc_code_destroy(code);
    return bad ? 5 : 0;
}
