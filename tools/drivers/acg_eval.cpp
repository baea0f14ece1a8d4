// N2 — evaluation driver: the reference's main.cpp:42-92 loop (decoder list x SNR list -> stdout + report.csv with
// the same header and 12-digit fixed precision, main.cpp:47-49,79-86) on the device.
//
//   acg_eval --H data/optimalH.txt [--G data/G05.txt] [--snrs -5,-4.5,...,0] [--tests 10000] [--bp-iters 100]
//            [--alpha 1.2 --mu 0.55 --admm-iters 10000 --eps 1e-5] [--noise host|device] [--seed 1] [--out report.csv]
//            [--gpus N]   (one decoder handle + host thread per GPU, contiguous frame ranges, counters summed)
//            [--minsum-iters N [--ms-scale 0.75] [--layered] [--ms-f16]]   also evaluate the build-added normalised min-sum
//                         (NOT in the reference: parity unpinned), flooding or with the layered schedule
//            [--detail [--detail-out report_detail.csv]]   also write post-decoding bit errors and the pseudo / non-codeword
//                         figures of every (decoder, SNR) through acg_ldpc_mc_run_detail
//            [--events-out FILE --events-cap N]   log the N lowest frames that are not correct, one line per event
//                         (a frame index replays the frame: device noise is keyed on it)
//            Without these three the driver runs acg_ldpc_mc_run and its output is what it always was.
//            [--cascade A,B]   A, B of bp | admm | minsum, the decoders the flags above configure: also evaluate the two-stage
//                         decoder "A then B on the frames A fails" (acg_ldpc_cascade_mc_run) on one device — one more block on
//                         stdout and one more row per SNR in report.csv, Method = the cascade's name (e.g. MS+BP), behind
//                         the rows of the single decoders; stderr adds the share of frames the second stage saw.  The
//                         detail files do not cover it.  Without the flag nothing changes.
//                         A, B may also be qms (the fixed-point layered min-sum with the default quantiser, --qms-iters N,
//                         default 25) and osd (order --osd-order, default 1); qms,osd hands the posteriors over.
//            [--osd-order K]   also evaluate ordered-statistics decoding of order K = 0 or 1 on the channel symbols (build-added;
//                         weak on its own on these codes: it is meant as the second stage behind qms)
//            [--qms-engine lds|streamed]   also evaluate the fixed-point layered min-sum on its own (default quantiser, --qms-iters N):
//                         lds = acg_ldpc_decoder_create_quantized (a frame in LDS), streamed =
//                         acg_ldpc_decoder_create_quantized_streamed (a frame in device memory: any code size, any check
//                         degree).  One more block, Method = QMS; both engines give the same rows.
//            [--layered-streamed bp|minsum|bp,minsum]   also evaluate the layered sum-product (--bp-iters) and / or the layered
//                         min-sum (--minsum-iters, --ms-scale) on the streamed float layered engine,
//                         acg_ldpc_decoder_create_layered_streamed (fp32 state in device memory: any code size, any check
//                         degree).  One more block each, Method = BP / MS, behind the others.
//            [--puncture LIST] [--shorten LIST]   LIST = comma-separated variable indices and a-b ranges: a rate-matched run
//                         (acg_ldpc_mc_run_rm) — the listed positions are not transmitted; a punctured one reaches the decoder
//                         as an erasure, a shortened one as a known bit; FER counts all n positions, the Hamming figures the
//                         sent ones; --snrs stay Es/N0 of a transmitted symbol.  Only together with --qms-engine and / or
//                         --qms-iters (alone: the LDS engine) and / or --layered-streamed, and with --noise device: those blocks alone are evaluated
//                         (no BP, QP-ADMM or flooding min-sum block); every other combination is refused before a device is
//                         looked for.  The output line format is unchanged.
// Defaults are main.cpp's (OPTIMAL build): optimalH, BP(100), QP-ADMM(1.2, 0.55, 10000, 1e-5), 10000 codewords from
// mt19937(239'239'239), SNRs -5..0 step 0.5.  --noise host reproduces the reference's frames bit for bit
// (frame i <- mt19937(i+1)); --noise device keeps generation, decoding and classification on the GPU.
#include <cmath>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "common.hpp"

int main(int argc, char **argv) {
    drv::Args a{argc, argv};
    const char *hpath = a.get("--H", "data/optimalH.txt");
    const int64_t tests = a.integer("--tests", 10000);                     // TESTS_NUM, main.cpp:25
    std::vector<double> snrs = drv::parse_list(a.get("--snrs", "-5,-4.5,-4,-3.5,-3,-2.5,-2,-1.5,-1,-0.5,0"));  // main.cpp:27
    const int noise = std::strcmp(a.get("--noise", "host"), "device") ? ACG_LDPC_NOISE_HOST_MT19937 : ACG_LDPC_NOISE_DEVICE_PHILOX;
    // detail run: checked before anything is loaded or launched
    const bool want_events = a.has("--events-out") || a.has("--events-cap");
    const bool detail = a.has("--detail") || a.has("--detail-out") || want_events;
    const int64_t events_cap = want_events ? a.integer("--events-cap", 0) : 0;
    if (want_events && (!a.get("--events-out") || events_cap <= 0)) {
        std::fprintf(stderr, "acg_eval: --events-out FILE and --events-cap N (N > 0) go together\n");
        return 2;
    }
    std::string cascade_first, cascade_second;
    if (a.has("--cascade")) {
        const std::string spec = a.get("--cascade", "");
        const size_t comma = spec.find(',');
        auto known = [](const std::string &w) { return w == "bp" || w == "admm" || w == "minsum" || w == "qms" || w == "osd"; };
        if (comma != std::string::npos) cascade_first = spec.substr(0, comma), cascade_second = spec.substr(comma + 1);
        if (!known(cascade_first) || !known(cascade_second)) {
            std::fprintf(stderr, "acg_eval: --cascade A,B with A and B of bp, admm, minsum, qms, osd\n");
            return 2;
        }
    }
    const std::string qms_engine = a.get("--qms-engine", "");
    if (a.has("--qms-engine") && qms_engine != "lds" && qms_engine != "streamed") {
        std::fprintf(stderr, "acg_eval: --qms-engine lds or streamed\n");
        return 2;
    }
    std::vector<std::string> layered_streamed;
    if (a.has("--layered-streamed")) {
        const std::string spec = a.get("--layered-streamed", "");
        if (spec == "bp" || spec == "minsum") layered_streamed = {spec};
        else if (spec == "bp,minsum") layered_streamed = {"bp", "minsum"};
        else {
            std::fprintf(stderr, "acg_eval: --layered-streamed bp, minsum or bp,minsum\n");
            return 2;
        }
    }
    // rate matching: checked before anything is loaded or a device is looked for
    const bool rm = a.has("--puncture") || a.has("--shorten");
    std::vector<long> punctured, shortened;
    if (rm) {
        if ((a.has("--puncture") && !drv::parse_index_list(a.get("--puncture", ""), punctured)) ||
            (a.has("--shorten") && !drv::parse_index_list(a.get("--shorten", ""), shortened))) {
            std::fprintf(stderr, "acg_eval: --puncture LIST / --shorten LIST with LIST of comma-separated indices and a-b ranges\n");
            return 2;
        }
        if (!a.has("--qms-engine") && !a.has("--qms-iters") && layered_streamed.empty()) {
            std::fprintf(stderr, "acg_eval: --puncture / --shorten need an engine with a channel-value entrance: --qms-engine lds|streamed "
                                 "[--qms-iters N] or --layered-streamed bp|minsum|bp,minsum\n");
            return 2;
        }
        if (a.has("--cascade") || a.has("--osd-order") || detail) {
            std::fprintf(stderr, "acg_eval: --puncture / --shorten do not go with --cascade, --osd-order or a detail run\n");
            return 2;
        }
        if (noise == ACG_LDPC_NOISE_HOST_MT19937) {
            std::fprintf(stderr, "acg_eval: --puncture / --shorten run with device noise only: pass --noise device\n");
            return 2;
        }
    }
    acg_ldpc_code *code = nullptr;
    if (acg_ldpc_code_load_txt(hpath, &code)) drv::die("read_pcm");
    int m, n, E;
    acg_ldpc_code_dims(code, &m, &n, &E);
    std::vector<uint8_t> pattern;
    if (rm) {
        pattern.assign((size_t) n, (uint8_t) ACG_LDPC_RM_SENT);
        for (int pass = 0; pass < 2; pass++)
            for (long v : pass ? shortened : punctured) {
                if (v >= n || pattern[(size_t) v] != ACG_LDPC_RM_SENT) {
                    std::fprintf(stderr, "acg_eval: --puncture / --shorten index %ld is %s\n", v, v >= n ? "outside the code" : "listed twice");
                    return 2;
                }
                pattern[(size_t) v] = (uint8_t) (pass ? ACG_LDPC_RM_SHORTENED : ACG_LDPC_RM_PUNCTURED);
            }
    }
    bool ok;
    std::vector<uint8_t> cws = drv::make_codewords(code, a.get("--G"), 239239239u, tests, &ok);  // main.cpp:63-64
    if (!ok) {
        std::fprintf(stderr, "GetOrtogonal failed for %s\n", hpath);
        return 1;
    }
    std::cerr << "n=" << n << " k=" << m << "\n";  // main.cpp:66 (prints H.size() as k)

    const int gpus = (int) a.integer("--gpus", 1);
    const int ndev = (int) a.integer("--device-count", 1 << 30);  // tests: fold N handles onto fewer devices
    std::vector<drv::MultiGpu> decs;
    // the three decoders the flags configure, by the names --cascade uses
    auto params_of = [&](const std::string &which, acg_ldpc_params &p) {
        acg_ldpc_params_default(&p);
        if (which == "bp") {
            p.algo = ACG_LDPC_BP_SUMPRODUCT;
            p.max_iter = (int) a.integer("--bp-iters", 100);  // main.cpp:29
        } else if (which == "admm") {
            p.algo = ACG_LDPC_QPADMM;
            p.alpha = a.num("--alpha", 1.2);  // main.cpp:31
            p.mu = a.num("--mu", 0.55);
            p.max_iter = (int) a.integer("--admm-iters", 10000);
            p.eps_stop = a.num("--eps", 1e-5);
        } else if (which == "minsum") {  // build-added variant (north_star); not one of main.cpp's decoders
            p.algo = ACG_LDPC_BP_MINSUM;
            p.max_iter = (int) a.integer("--minsum-iters", 50);
            p.ms_scale = a.num("--ms-scale", 0.75);
            if (a.has("--layered")) p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
            if (a.has("--ms-f16")) p.precision = ACG_LDPC_PREC_F16;
        } else if (which == "qms") {  // build-added fixed-point layered min-sum, default quantiser (cascades, --qms-engine)
            p.algo = ACG_LDPC_BP_MINSUM;
            p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
            p.max_iter = (int) a.integer("--qms-iters", 25);
        } else if (which == "osd") {  // build-added ordered-statistics decoding: max_iter is the order
            p.algo = ACG_LDPC_OSD;
            p.max_iter = (int) a.integer("--osd-order", 1);
        } else
            return false;
        return true;
    };
    // (a rate-matched run evaluates the engines with a channel-value entrance only: no BP, QP-ADMM or flooding min-sum block)
    acg_ldpc_params p;
    if (!rm && !a.has("--no-bp")) {
        params_of("bp", p);
        decs.emplace_back();
        decs.back().create(code, p, gpus, ndev);
    }
    if (!rm && !a.has("--no-admm")) {
        params_of("admm", p);
        decs.emplace_back();
        decs.back().create(code, p, gpus, ndev);
    }
    if (!rm && a.has("--minsum-iters")) {
        params_of("minsum", p);
        decs.emplace_back();
        decs.back().create(code, p, gpus, ndev);
    }
    if (a.has("--osd-order")) {
        params_of("osd", p);
        decs.emplace_back();
        decs.back().create(code, p, gpus, ndev);
    }
    if (a.has("--qms-engine") || (rm && a.has("--qms-iters"))) {   // (rate-matched: --qms-iters alone means the LDS engine)
        params_of("qms", p);
        acg_ldpc_quant q;
        acg_ldpc_quant_default(&q);
        decs.emplace_back();
        decs.back().create(code, p, gpus, ndev, &q, qms_engine == "streamed");
    }
    for (const std::string &which : layered_streamed) {
        params_of(which, p);
        p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
        p.precision = ACG_LDPC_PREC_DEFAULT;
        decs.emplace_back();
        decs.back().create(code, p, gpus, ndev, nullptr, false, true);
    }
    acg_ldpc_cascade *cascade = nullptr;
    if (a.has("--cascade")) {
        acg_ldpc_params p1, p2;
        params_of(cascade_first, p1);
        params_of(cascade_second, p2);
        acg_ldpc_quant q;
        acg_ldpc_quant_default(&q);
        if (acg_ldpc_cascade_create(code, &p1, cascade_first == "qms" ? &q : nullptr, &p2, cascade_second == "qms" ? &q : nullptr, &cascade))
            drv::die("acg_ldpc_cascade_create");
    }

    std::cout.precision(5);
    std::cout << std::fixed;
    std::ofstream fdata(a.get("--out", "report.csv"));
    fdata << "Method,SNR,Sigma,FER,Time,AvgHamming,AvgHammingCorrect,AvgHammingWrong" << std::endl;  // main.cpp:48
    fdata << std::fixed << std::setprecision(12);
    std::ofstream fdetail, fevents;
    if (detail) {
        fdetail.open(a.get("--detail-out", "report_detail.csv"));
        fdetail << "Method,SNR,Frames,FER,BER,WordFrames,BitErrors,Pseudo,MinPseudoWeight,MinPseudoFrame,NonCodewordFrames,AvgSyndromeWeight" << std::endl;
        fdetail << std::fixed << std::setprecision(12);
    }
    if (want_events) {
        fevents.open(a.get("--events-out"));
        fevents << "Method,SNR,Frame,Kind,Iters,RawErrors,BitErrors,SyndromeWeight" << std::endl;
    }
    for (double snr : snrs) std::cerr << "snr=" << snr << ": var=" << acg_ldpc_llr_variance(snr) << std::endl;
    for (auto &d : decs) {
        std::cout << "Algo: " << d.name() << std::endl;
        for (double snr : snrs) {
            drv::McOut r;
            if (detail) {
                drv::DetailOut dt = d.run_detail(cws, n, snr, tests, noise, (uint64_t) a.integer("--seed", 1), events_cap);
                r.r = dt.d.base;
                fdetail << d.name() << "," << snr << "," << dt.d.base.total << "," << dt.fer() << "," << dt.ber(n) << "," << dt.d.word_frames
                        << "," << dt.d.bit_errors << "," << dt.d.base.pseudo << "," << dt.d.min_pseudo_weight << ","
                        << dt.d.min_pseudo_frame << "," << dt.d.noncodeword_frames << "," << dt.avg_syndrome_weight() << std::endl;
                for (const acg_ldpc_mc_event &e : dt.events)
                    fevents << d.name() << "," << snr << "," << e.frame << "," << drv::event_kind_name(e.kind) << "," << e.iters << ","
                            << e.raw_errors << "," << e.bit_errors << "," << e.syndrome_weight << std::endl;
            } else
                r = d.run(cws, n, snr, tests, noise, (uint64_t) a.integer("--seed", 1), rm ? &pattern : nullptr);
            std::cout << "\tSNR: " << snr << ", FER: " << r.fer() << ", (time=" << r.avg_time() << "s)" << std::endl;
            std::cerr << "\t\tAverage hamming distance: " << r.mean_hamming() << std::endl;
            fdata << d.name() << "," << snr << "," << std::sqrt(acg_ldpc_llr_variance(snr)) << "," << r.fer() << ","
                  << r.avg_time() << "," << r.mean_hamming() << "," << r.mean_hamming_ok() << ","
                  << r.mean_hamming_wrong() << std::endl;
        }
        std::cerr << std::string(30, '_') << std::endl;
    }
    if (cascade) {
        std::cout << "Algo: " << acg_ldpc_cascade_name(cascade) << std::endl;
        for (double snr : snrs) {
            acg_ldpc_mc_cfg cfg;
            std::memset(&cfg, 0, sizeof cfg);
            cfg.frames = tests;
            cfg.snr = snr;
            cfg.seed = (uint64_t) a.integer("--seed", 1);
            cfg.noise = noise;
            cfg.codewords = cws.empty() ? nullptr : cws.data();
            cfg.n_codewords = cws.empty() ? 0 : (int64_t) (cws.size() / (size_t) n);
            acg_ldpc_cascade_result cr;
            if (acg_ldpc_cascade_mc_run(cascade, &cfg, &cr)) drv::die("acg_ldpc_cascade_mc_run");
            drv::McOut r, r1;
            r.r = cr.total;
            r1.r = cr.first;
            std::cout << "\tSNR: " << snr << ", FER: " << r.fer() << ", (time=" << r.avg_time() << "s)" << std::endl;
            std::cerr << "\t\tAverage hamming distance: " << r.mean_hamming() << std::endl;
            std::cerr << "\t\tFirst stage alone: FER " << r1.fer() << "; second stage: " << cr.second_frames << " of " << cr.total.total
                      << " frames, " << cr.second_correct << " decoded correctly" << std::endl;
            fdata << acg_ldpc_cascade_name(cascade) << "," << snr << "," << std::sqrt(acg_ldpc_llr_variance(snr)) << "," << r.fer() << ","
                  << r.avg_time() << "," << r.mean_hamming() << "," << r.mean_hamming_ok() << "," << r.mean_hamming_wrong() << std::endl;
        }
        std::cerr << std::string(30, '_') << std::endl;
        acg_ldpc_cascade_destroy(cascade);
    }
    for (auto &d : decs) d.destroy();
    acg_ldpc_code_destroy(code);
    return 0;
}
