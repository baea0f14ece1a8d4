// Compiled and, on a GPU box, run by tests/test_streamed_layered_io_gpu.py (tests/test_streamed_layered_io.py compiles it and
// runs it without a device): the LLR entrance's members of acg_ldpc::StreamedLayeredBPDecoder / StreamedLayeredMinSumDecoder of
// include/acg_ldpc_decoder.hpp must compile with plain g++ against include/, and on the LLRs the symbol entrance forms from
// its symbols return the words and flags the symbol entrance returns, with posteriors whose sign bits are the words.
#include <cmath>
#include <cstdio>
#include <string>

#include "acg_ldpc_decoder.hpp"

using namespace acg_ldpc;

template <class Dec>
static int run(Dec &dec, const TMatrix &H, const std::vector<double> &y, const std::vector<float> &L, double snr, int n) {
    const auto sym = dec.decode_batch(H, y, snr);
    const auto r = dec.decode_llr_batch(H, L);
    const auto plain = dec.decode_llr_batch(H, L, false);
    int same = plain.post.empty() && plain.bits == r.bits && plain.ok == r.ok && r.post.size() == L.size(), sign_mismatch = 0;
    for (size_t f = 0; f < sym.size(); f++) {
        same = same && (r.ok[f] != 0) == sym[f].second;
        for (int v = 0; v < n && r.ok[f]; v++) {
            same = same && r.bits[f * n + v] == sym[f].first[v];
            sign_mismatch += std::signbit(r.post[f * n + v]) != (r.bits[f * n + v] != 0);
        }
    }
    std::printf("%s frames=%zu same=%d sign_mismatch=%d ok=%d,%d\n", dec.name().c_str(), sym.size(), same, sign_mismatch, (int) r.ok[0], (int) r.ok[1]);
    return same && !sign_mismatch ? 0 : 1;
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
    float one = 0;
    uint8_t out = 0;
    const int rc = acg_ldpc_decode_batch_llr(nullptr, &one, 1, &out, &out, nullptr, nullptr);
    std::printf("m=%d n=%d E=%d null handle: %s\n", m, n, E, rc ? acg_ldpc_last_error() : "accepted");
    if (rc == 0) return 4;
    StreamedLayeredBPDecoder bp(15);
    StreamedLayeredMinSumDecoder ms(15, 0.75);
    if (!acg_ldpc_device_available()) {
        std::printf("no device: compile/link check only\n");
        return 0;
    }
    // the all-zero word (symbol +1) under a fixed pattern of noise, two frames, the second noisier, and the LLRs the symbol
    // entrance forms from double symbols: (float) (2 y / sigma^2)
    const double snr = 1.0, var = acg_ldpc_llr_variance(snr);
    std::vector<double> y((size_t) 2 * n);
    std::vector<float> L(y.size());
    for (size_t i = 0; i < y.size(); i++) {
        const double u = (double) ((uint32_t) (i * 2654435761u) >> 8) / 16777216.0 - 0.5;   // -0.5 ... 0.5
        y[i] = 1.0 + (i < (size_t) n ? 2.2 : 3.4) * u;
        L[i] = (float) (2 * y[i] / var);
    }
    int bad = run(bp, H, y, L, snr, n) + run(ms, H, y, L, snr, n);
    char text[1024];
    acg_ldpc_decoder_describe(bp.handle(H), text, (int32_t) sizeof text);
    std::printf("%s\n", text);
    acg_ldpc_code_destroy(code);
    return bad ? 5 : 0;
}
