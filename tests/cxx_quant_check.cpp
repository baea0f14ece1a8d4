// Compiled (and, on a GPU box, run) by tests/test_layered_q_gpu.py: QuantizedMinSumDecoder of include/acg_ldpc_decoder.hpp, the C++
// mirror of the fixed-point layered min-sum engine, must compile with plain g++ against include/ and decode like the other mirrors.
#include <cstdio>
#include <memory>
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
    acg_ldpc_quant q = QuantizedMinSumDecoder::default_quant();
    std::printf("m=%d n=%d E=%d quant=%g,%d,%d,%d,%d,%d,%d check=%d sizeof=%zu\n", m, n, E, q.llr_step, q.ch_bits, q.msg_bits, q.post_bits,
                q.scale_num, q.scale_shift, q.offset, acg_ldpc_quant_check(&q), sizeof(acg_ldpc_quant));
    q.msg_bits = 9;
    if (acg_ldpc_quant_check(&q) == 0) return 4;
    std::shared_ptr<Decoder> dec = std::make_shared<QuantizedMinSumDecoder>(20);
    std::printf("name=%s\n", dec->name().c_str());
    if (!acg_ldpc_device_available()) {
        std::printf("no device: compile/link check only\n");
        return 0;
    }
    std::vector<uint8_t> G((size_t) (n - m) * n), cw((size_t) n);
    if (acg_ldpc_code_generator(code, G.data())) return 4;
    acg_ldpc_gen_codewords(G.data(), n - m, n, 239239239u, 1, cw.data());
    TFVector y((size_t) n);
    for (int i = 0; i < n; i++) y[(size_t) i] = cw[(size_t) i] ? -1.0 : 1.0;   // noiseless
    auto p = dec->decode(H, y, 0.0);
    int diff = 0;
    if (p.second)
        for (int i = 0; i < n; i++) diff += (p.first[i] != (bool) cw[i]);
    std::printf("%s noiseless ok=%d size=%zu diff=%d\n", dec->name().c_str(), (int) p.second, p.first.size(), diff);
    if (!p.second || diff) return 5;
    // hopeless word (channel values -2 and +2 at -5 dB; tests/layered_q_ref.py fails it after 20 iterations): the EMPTY vector +
    // false, as the BP mirrors return it
    TFVector bad((size_t) n, -0.8);
    for (int i = 0; i < n; i += 3) bad[i] = 1.0;
    p = dec->decode(H, bad, -5.0);
    std::printf("%s hopeless ok=%d size=%zu\n", dec->name().c_str(), (int) p.second, p.first.size());
    if (p.second || !p.first.empty()) return 6;
    char text[1024];
    acg_ldpc_decoder_describe(static_cast<QuantizedMinSumDecoder *>(dec.get())->handle(H), text, (int32_t) sizeof text);
    std::printf("%s\n", text);
    acg_ldpc_code_destroy(code);
    return 0;
}
