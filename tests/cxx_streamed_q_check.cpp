// Compiled by tests/test_streamed_q_cabi.py and, on a GPU box, run by tests/test_streamed_q_gpu.py: StreamedQuantizedMinSumDecoder of
// include/acg_ldpc_decoder.hpp must compile with plain g++ against include/ and return what QuantizedMinSumDecoder returns.
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
    StreamedQuantizedMinSumDecoder dec(15);
    QuantizedMinSumDecoder lds(15);
    std::printf("m=%d n=%d E=%d name=%s\n", m, n, E, dec.name().c_str());
    acg_ldpc_params p;
    acg_ldpc_params_default(&p);
    p.algo = ACG_LDPC_BP_MINSUM;
    p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
    p.engine = ACG_LDPC_ENGINE_FUSED;
    acg_ldpc_quant q = QuantizedMinSumDecoder::default_quant();
    acg_ldpc_decoder *d = nullptr;
    const int rc = acg_ldpc_decoder_create_quantized_streamed(code, &p, &q, &d);
    std::printf("fused: rc=%d %s\n", rc != 0, acg_ldpc_last_error());
    if (rc == 0) return 4;
    if (!acg_ldpc_device_available()) {
        std::printf("no device: compile/link check only\n");
        return 0;
    }
    // channel values of a fixed pattern, two frames: both engines return the same words, flags, iterations and posteriors
    std::vector<int16_t> c((size_t) 2 * n);
    for (size_t i = 0; i < c.size(); i++) c[i] = (int16_t) ((int) ((i * 2654435761u) >> 27) - (i < (size_t) n ? 6 : 14));
    auto a = dec.decode_llr_batch(H, c), b = lds.decode_llr_batch(H, c);
    const bool same = a.bits == b.bits && a.ok == b.ok && a.iters == b.iters && a.post == b.post;
    std::printf("same=%d ok=%d,%d iters=%d,%d\n", (int) same, (int) a.ok[0], (int) a.ok[1], a.iters[0], a.iters[1]);
    if (!same) return 5;
    char text[1024];
    acg_ldpc_decoder_describe(dec.handle(H), text, (int32_t) sizeof text);
    std::printf("%s\n", text);
    acg_ldpc_code_destroy(code);
    return 0;
}
