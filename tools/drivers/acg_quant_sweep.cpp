// Format search of the fixed-point layered min-sum engine: the cross product of one list per quantiser field, scored in ONE
// acg_ldpc_mc_run_quants call on one handle of acg_ldpc_decoder_create_quantized.
//   acg_quant_sweep [--H data/H05.txt] [--G <generator file>] [--snr -2] [--tests 1000] [--iters 25] [--lanes 0]
//                   [--noise host|device] [--seed 1]
//                   [--llr-step 0.5] [--ch-bits 6] [--msg-bits 6] [--post-bits 8] [--scale-num 1] [--scale-shift 0] [--offset 1]
// Every quantiser option takes a comma-separated list (--ch-bits 4,5,6); the defaults are acg_ldpc_quant_default's.  The lists
// are crossed in the order above (the last one fastest).  Combinations that acg_ldpc_quant_check rejects — ch_bits above
// post_bits, an offset above Rmax, ... — are dropped and their number goes to stderr.  Codewords: those of the generator
// file, or of G = the orthogonal complement of H, from mt19937(239) as the other drivers make them.
// stdout: a CSV, one row per surviving point in that order, 12-digit fixed precision like acg_eval's report:
//   llr_step,ch_bits,msg_bits,post_bits,scale_num,scale_shift,offset,fer,pseudo_rate,mean_iters
#include <iomanip>
#include <iostream>

#include "common.hpp"

int main(int argc, char **argv) {
    drv::Args a{argc, argv};
    const char *hpath = a.get("--H", "data/H05.txt");
    const int64_t tests = a.integer("--tests", 1000);
    const double snr = a.num("--snr", -2.0);
    const int noise = std::strcmp(a.get("--noise", "host"), "device") ? ACG_LDPC_NOISE_HOST_MT19937 : ACG_LDPC_NOISE_DEVICE_PHILOX;
    acg_ldpc_quant def;
    acg_ldpc_quant_default(&def);
    auto list = [&](const char *key, double dflt) {
        const char *v = a.get(key);
        std::vector<double> l = v ? drv::parse_list(v) : std::vector<double>{dflt};
        if (l.empty()) {
            std::fprintf(stderr, "%s: empty list\n", key);
            std::exit(1);
        }
        return l;
    };
    const std::vector<double> steps = list("--llr-step", def.llr_step), chs = list("--ch-bits", def.ch_bits), msgs = list("--msg-bits", def.msg_bits),
                              posts = list("--post-bits", def.post_bits), nums = list("--scale-num", def.scale_num),
                              shifts = list("--scale-shift", def.scale_shift), offs = list("--offset", def.offset);
    std::vector<acg_ldpc_quant> quants;
    long dropped = 0;
    for (double st : steps)
        for (double ch : chs)
            for (double ms : msgs)
                for (double po : posts)
                    for (double nu : nums)
                        for (double sh : shifts)
                            for (double of : offs) {
                                const acg_ldpc_quant q{st, (int32_t) ch, (int32_t) ms, (int32_t) po, (int32_t) nu, (int32_t) sh, (int32_t) of};
                                if (acg_ldpc_quant_check(&q)) dropped++;
                                else quants.push_back(q);
                            }
    std::cerr << "points=" << quants.size() << " dropped=" << dropped << " (rejected by acg_ldpc_quant_check)" << std::endl;
    if (quants.empty()) return 1;
    acg_ldpc_code *code = nullptr;
    if (acg_ldpc_code_load_txt(hpath, &code)) drv::die("read_pcm");
    int m, n, E;
    acg_ldpc_code_dims(code, &m, &n, &E);
    bool ok;
    std::vector<uint8_t> cws = drv::make_codewords(code, a.get("--G"), 239u, tests, &ok);
    if (!ok) return 1;
    acg_ldpc_params p;
    acg_ldpc_params_default(&p);
    p.algo = ACG_LDPC_BP_MINSUM;
    p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
    p.max_iter = (int32_t) a.integer("--iters", 25);
    p.lanes_per_frame = (int32_t) a.integer("--lanes", 0);
    acg_ldpc_decoder *d = nullptr;
    if (acg_ldpc_decoder_create_quantized(code, &p, &quants[0], &d)) drv::die("acg_ldpc_decoder_create_quantized");
    acg_ldpc_mc_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.frames = tests;
    cfg.snr = snr;
    cfg.seed = (uint64_t) a.integer("--seed", 1);
    cfg.noise = noise;
    cfg.codewords = cws.empty() ? nullptr : cws.data();
    cfg.n_codewords = cws.empty() ? 0 : (int64_t) (cws.size() / (size_t) n);
    std::vector<acg_ldpc_mc_result> res(quants.size());
    if (acg_ldpc_mc_run_quants(d, &cfg, quants.data(), (int32_t) quants.size(), res.data())) drv::die("acg_ldpc_mc_run_quants");
    acg_ldpc_decoder_destroy(d);
    acg_ldpc_code_destroy(code);
    std::cout << "llr_step,ch_bits,msg_bits,post_bits,scale_num,scale_shift,offset,fer,pseudo_rate,mean_iters\n";
    std::cout << std::fixed << std::setprecision(12);
    for (size_t k = 0; k < quants.size(); k++) {
        const acg_ldpc_quant &q = quants[k];
        const acg_ldpc_mc_result &r = res[k];
        const double tot = (double) (r.total > 0 ? r.total : 1);
        std::cout << q.llr_step << "," << q.ch_bits << "," << q.msg_bits << "," << q.post_bits << "," << q.scale_num << "," << q.scale_shift << ","
                  << q.offset << "," << (double) (r.total - r.correct) / tot << "," << (double) r.pseudo / tot << "," << (double) r.sum_iters / tot << "\n";
    }
    return 0;
}
