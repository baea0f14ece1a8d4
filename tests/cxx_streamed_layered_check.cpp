// Compiled by tests/test_streamed_layered_cabi.py and, on a GPU box, run by tests/test_streamed_layered_gpu.py:
// StreamedLayeredBPDecoder and StreamedLayeredMinSumDecoder of include/acg_ldpc_decoder.hpp must compile with plain g++ against
// include/ and return what the LDS layered classes (one workgroup of 256 threads per frame) return.
#include <cstdio>
#include <string>

#include "acg_ldpc_decoder.hpp"

using namespace acg_ldpc;

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
    StreamedLayeredBPDecoder bp(15);
    StreamedLayeredMinSumDecoder ms(15, 0.75);
    BeliefPropagationDecoder bp_lds(15, true, 256);
    MinSumDecoder ms_lds(15, 0.75, true, 256);
    std::printf("m=%d n=%d E=%d names=%s,%s\n", m, n, E, bp.name().c_str(), ms.name().c_str());
    acg_ldpc_params p;
    acg_ldpc_params_default(&p);
    p.algo = ACG_LDPC_BP_SUMPRODUCT;
    p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
    p.engine = ACG_LDPC_ENGINE_FUSED;
    acg_ldpc_decoder *d = nullptr;
    const int rc = acg_ldpc_decoder_create_layered_streamed(code, &p, &d);
    std::printf("fused: rc=%d %s\n", rc != 0, acg_ldpc_last_error());
    if (rc == 0) return 4;
    if (!acg_ldpc_device_available()) {
        std::printf("no device: compile/link check only\n");
        return 0;
    }
    // the all-zero word (symbol +1) under a fixed pattern of noise, two frames, the second noisier: both engines return the same
    // words and flags
    std::vector<double> y((size_t) 2 * n);
    for (size_t i = 0; i < y.size(); i++) {
        const double u = (double) ((uint32_t) (i * 2654435761u) >> 8) / 16777216.0 - 0.5;   // -0.5 ... 0.5
        y[i] = 1.0 + (i < (size_t) n ? 2.2 : 3.4) * u;
    }
    const double snr = 1.0;
    auto a = bp.decode_batch(H, y, snr), b = bp_lds.decode_batch(H, y, snr);
    auto c = ms.decode_batch(H, y, snr), e = ms_lds.decode_batch(H, y, snr);
    const bool same = a == b && c == e;
    std::printf("same=%d bp ok=%d,%d ms ok=%d,%d\n", (int) same, (int) a[0].second, (int) a[1].second, (int) c[0].second, (int) c[1].second);
    if (!same) return 5;
    char text[1024];
    acg_ldpc_decoder_describe(bp.handle(H), text, (int32_t) sizeof text);
    std::printf("%s\n", text);
    acg_ldpc_decoder_describe(ms.handle(H), text, (int32_t) sizeof text);
    std::printf("%s\n", text);
    acg_ldpc_decoder_describe(bp_lds.handle(H), text, (int32_t) sizeof text);
    std::printf("%s\n", text);
    acg_ldpc_code_destroy(code);
    return 0;
}
