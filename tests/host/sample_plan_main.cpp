// Stand-alone driver of csrc/tld_sample_plan.h (the checks, the plan and the staged upload of one sampler call), built by
// tests/test_sample_plan_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     sample_plan_main CASES.txt
//
// CASES.txt holds one call per line, whitespace-separated; floats travel as the hex bit patterns of their float32 values, so a NaN or a sigma that
// differs in its last bit arrives as written:
//     name entry B n_max stride has_mask has_init has_neg_labels guidance_skip max_batch
//          R n_rec (n_levels g mix has_negative) x n_rec       C n (bits) x n       G n (bits) x n       E n (bits) x n       K n (u64 hex) x n       S n (bits) x n
// A count of -1 stands for a null pointer.  Per call the driver prints one JSON object on one line: the refusal of sample_call_check; if there is
// none, the refusal of sample_plan; if there is none, every field of the plan and the bytes sample_plan_fill wrote into a buffer of exactly
// plan.stage_bytes that held 0xCD before (hex).  The plan object is reused from call to call, as the engine reuses its own.
#include "tld_sample_plan.h"

#include <cinttypes>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

using namespace tld;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// "X n v v v": false where n is -1 (a null pointer)
static bool read_floats(std::istringstream& in, const char* tag, std::vector<float>& out) {
    std::string t; long n;
    in >> t >> n;
    if (t != tag) { std::fprintf(stderr, "expected %s, got %s\n", tag, t.c_str()); std::exit(2); }
    out.clear();
    for (long k = 0; k < n; ++k) { std::string h; in >> h; out.push_back(from_bits((uint32_t)std::strtoul(h.c_str(), nullptr, 16))); }
    return n >= 0;
}

static std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
    return o + "\"";
}

template <class T> static void print_ints(const char* key, const std::vector<T>& v) {
    std::printf(", \"%s\": [", key);
    for (size_t k = 0; k < v.size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)v[k]);
    std::printf("]");
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES.txt\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    SamplePlan plan;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string name;
        if (!(in >> name)) continue;
        SampleCall c{};
        int entry, has_mask, has_init, has_neg, skip;
        in >> entry >> c.B >> c.n_max >> c.stride >> has_mask >> has_init >> has_neg >> skip >> c.max_batch;
        c.entry = (SampleEntry)entry; c.has_mask = has_mask; c.has_init = has_init; c.has_neg_labels = has_neg; c.guidance_skip = skip;
        std::string t; long n_rec;
        in >> t >> n_rec;
        std::vector<tld_sample_request> recs;
        for (long k = 0; k < n_rec; ++k) {
            tld_sample_request r; std::string g, m;
            in >> r.n_levels >> g >> m >> r.has_negative;
            r.class_guidance = from_bits((uint32_t)std::strtoul(g.c_str(), nullptr, 16)); r.start_mix = from_bits((uint32_t)std::strtoul(m.c_str(), nullptr, 16));
            recs.push_back(r);
        }
        std::vector<float> coeffs, guidance, noise_coeff, shape;
        std::vector<uint64_t> keys;
        c.requests = n_rec >= 0 ? recs.data() : nullptr;
        c.coeffs = read_floats(in, "C", coeffs) ? coeffs.data() : nullptr;
        c.guidance = read_floats(in, "G", guidance) ? guidance.data() : nullptr;
        c.noise_coeff = read_floats(in, "E", noise_coeff) ? noise_coeff.data() : nullptr;
        long n_keys;
        in >> t >> n_keys;
        for (long k = 0; k < n_keys; ++k) { std::string h; in >> h; keys.push_back(std::strtoull(h.c_str(), nullptr, 16)); }
        c.noise_keys = n_keys >= 0 ? keys.data() : nullptr;
        c.shape = read_floats(in, "S", shape) ? shape.data() : nullptr;
        if (!in) { std::fprintf(stderr, "%s: a short line\n", name.c_str()); return 2; }

        std::printf("{\"name\": %s", quoted(name).c_str());
        const SampleRefusal bad = sample_call_check(c);
        std::printf(", \"check\": [%d, %s]", bad.code, quoted(bad.msg).c_str());
        if (!bad) {
            const SampleRefusal full = sample_plan(c, plan);
            std::printf(", \"plan\": [%d, %s]", full.code, quoted(full.msg).c_str());
            if (!full) {
                const SamplePlan& p = plan;
                std::printf(", \"slots\": %d, \"noise\": %d, \"shape\": %d, \"skip\": %d, \"B\": %d, \"n_max\": %d, \"stride\": %d, \"tabB\": %d, \"per\": %d", p.slots,
                            p.noise, p.shape, p.skip, p.B, p.n_max, p.stride, p.tabB, p.per);
                std::printf(", \"Tn\": %d, \"n_neg\": %d, \"T\": %d, \"rows_cond\": %lld, \"rows_uncond\": %lld, \"any_mix\": %d, \"any_shape\": %d, \"any_mom\": %d", p.Tn,
                            p.n_neg, p.T, (long long)p.rows_cond, (long long)p.rows_uncond, p.any_mix, p.any_shape, p.any_mom);
                std::printf(", \"mix_off\": %zu, \"rows_off\": %zu, \"noise_off\": %zu, \"shape_off\": %zu, \"up_bytes\": %zu, \"stage_bytes\": %zu", p.mix_off, p.rows_off,
                            p.noise_off, p.shape_off, p.up_bytes, p.stage_bytes);
                std::vector<long long> Bi, U, mb, off, stats, slot, sig;
                for (const SampleStep& s : p.steps) { Bi.push_back(s.Bi); U.push_back(s.U); mb.push_back(s.mb); off.push_back((long long)s.rows_off); stats.push_back(s.stats); }
                for (int i = 0; i < p.n_max; ++i)                  // (the slots and sigma rows of the requests still running; the rest of a row is not the plan's)
                    for (int b = 0; b < p.B; ++b) slot.push_back(b < p.steps[(size_t)i].Bi ? p.slot[(size_t)i * p.B + b] : -2);
                for (float s : p.sig) sig.push_back(to_bits(s));
                print_ints("Bi", Bi); print_ints("U", U); print_ints("mb", mb); print_ints("step_rows_off", off); print_ints("stats", stats);
                print_ints("slot", slot); print_ints("sig", sig); print_ints("noise_idx", p.noise_idx);
                unsigned char* buf = static_cast<unsigned char*>(std::malloc(p.stage_bytes));      // exactly: a write past the end is the sanitizer's
                memset(buf, 0xCD, p.stage_bytes);
                sample_plan_fill(p, c, buf);
                std::printf(", \"bytes\": \"");
                for (size_t k = 0; k < p.stage_bytes; ++k) std::printf("%02x", buf[k]);
                std::printf("\"");
                std::free(buf);
            }
        }
        std::printf("}\n");
    }
    return 0;
}
