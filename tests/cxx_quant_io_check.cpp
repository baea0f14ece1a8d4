// Compiled (and, on a GPU box, run) by tests/test_layered_q_io_gpu.py: the integer entrance of acg_ldpc::QuantizedMinSumDecoder
// (include/acg_ldpc_decoder.hpp) — quantize, decode_llr_batch with and without posteriors, and the no-op form of the two device
// members — with plain g++ against include/.
//   cxx_quant_io_check H.txt max_iter snr symbols.bin out.bin
// symbols.bin: frames*n doubles.  out.bin: frames*n int16 channel values | frames*n bytes | frames flags | frames int32 iterations
// | frames*n int16 posteriors, for the test to compare with the Python mirror and the restatement.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "acg_ldpc_decoder.hpp"

using namespace acg_ldpc;

template <class T>
static bool put(std::FILE *f, const std::vector<T> &v) {
    return std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
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
    acg_ldpc_code_destroy(code);
    TMatrix H(m, TCodeword(n));
    for (int i = 0; i < m; i++)
        for (int j = 0; j < n; j++) H[i][j] = dense[(size_t) i * n + j];
    // the three entry points refuse a null handle wherever they run
    int16_t one = 0;
    uint8_t b = 0;
    if (!acg_ldpc_decode_batch_q(nullptr, &one, 1, &b, &b, nullptr, nullptr) || !acg_ldpc_decode_batch_q_dev(nullptr, &one, 1, nullptr, nullptr, nullptr, nullptr, nullptr) ||
        !acg_ldpc_quantize_dev(nullptr, &one, 1, 1, 0.0, &one, nullptr))
        return 4;
    std::printf("m=%d n=%d E=%d null handle: %s\n", m, n, E, acg_ldpc_last_error());
    if (!acg_ldpc_device_available() || argc < 6) {
        std::printf("no device: compile/link check only\n");
        return 0;
    }
    const int max_iter = std::atoi(argv[2]);
    const double snr = std::atof(argv[3]);
    std::vector<double> Y;
    {
        std::FILE *f = std::fopen(argv[4], "rb");
        if (!f) return 5;
        double buf[4096];
        for (size_t k; (k = std::fread(buf, sizeof(double), 4096, f)) > 0;) Y.insert(Y.end(), buf, buf + k);
        std::fclose(f);
    }
    const size_t frames = Y.size() / (size_t) n;
    if (frames == 0 || Y.size() != frames * (size_t) n) return 5;
    QuantizedMinSumDecoder dec(max_iter);
    const std::vector<int16_t> c = dec.quantize(Y, snr);
    QuantizedMinSumDecoder::LlrResult r = dec.decode_llr_batch(H, c), r0 = dec.decode_llr_batch(H, c, false);
    if (r.post.size() != frames * (size_t) n || !r0.post.empty() || r0.bits != r.bits || r0.ok != r.ok || r0.iters != r.iters) return 6;
    // no frames, no symbols: both device members return without a launch
    dec.decode_llr_batch_dev(H, nullptr, 0, nullptr, nullptr);
    dec.quantize_dev(H, nullptr, true, 0, snr, nullptr);
    size_t good = 0, sign = 0;
    for (size_t f = 0; f < frames; f++) {
        good += r.ok[f];
        if (r.ok[f])
            for (int v = 0; v < n; v++) sign += (r.post[f * n + v] < 0) != (r.bits[f * n + v] != 0);
    }
    std::printf("%s frames=%zu ok=%zu sign_mismatch=%zu handles=%zu\n", dec.name().c_str(), frames, good, sign, dec.live_handles());
    std::FILE *o = std::fopen(argv[5], "wb");
    if (!o) return 7;
    const bool w = put(o, c) && put(o, r.bits) && put(o, r.ok) && put(o, r.iters) && put(o, r.post);
    return std::fclose(o) == 0 && w ? 0 : 7;
}
