// Stand-alone driver of csrc/tld_session_plan.h (the slot and row tables of a sampler session and the staged upload of every step), built by
// tests/test_session_plan_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     session_plan_main SCRIPT.txt
//
// SCRIPT.txt holds one command per line, whitespace-separated; floats travel as the hex bit patterns of their float32 values:
//     open slots cond_rows skip max_batch
//     admit n_levels g has_negative has_neg_label reserved   C n (bits) x n   G n (bits) x n   E n (bits) x n   K n (u64 hex) x n
//     step
// A count of -1 stands for a null pointer.  Per command the driver prints one JSON object on one line.  open: the refusal of session_open_check.
// admit: the refusal of session_request_check; if there is none, that of session_admit, the slot, the new sigma rows and the label rows.  step: the
// sizes, the finished slots and the bytes session_step wrote into a buffer of exactly max_up_bytes() that held 0xCD before (hex, up_bytes of them;
// "tail": whether every byte behind them still holds 0xCD), and "solo": whether every emitted row equals the row sample_plan_fill writes for that
// request alone at that forward -- g, a, b, c, c1, c2 and s_next by their bits, the final bit, whether the forward has an unconditional sample, and
// e / key.  The solo plans are made here with the existing header.  admit and step end with the session's whole state.
#include "tld_session_plan.h"

#include <cinttypes>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

using namespace tld;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

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

// the request alone, as a call of the entry its operands select: its plan and its upload
struct Solo {
    SamplePlan plan;
    std::vector<unsigned char> bytes;
    bool ok = false;
};

static void make_solo(const tld_session_request& r, bool skip, Solo& s) {
    tld_sample_request rec{r.n_levels, r.class_guidance, 1.0f, r.has_negative};
    SampleCall c{};
    c.entry = r.noise_coeff ? SE_STOCHASTIC : r.guidance ? SE_GUIDED : SE_REQUESTS;
    c.B = 1; c.n_max = r.n_levels; c.stride = 1; c.requests = &rec; c.coeffs = r.coeffs; c.guidance = r.guidance; c.noise_coeff = r.noise_coeff;
    c.noise_keys = r.noise_key; c.has_neg_labels = r.has_negative != 0; c.guidance_skip = skip; c.max_batch = 2;
    s.ok = !sample_call_check(c) && !sample_plan(c, s.plan);
    if (!s.ok) return;
    s.bytes.assign(s.plan.stage_bytes, 0);
    sample_plan_fill(s.plan, c, s.bytes.data());
}

static void print_state(const SessionPlan& p, long long solo_cond, long long solo_uncond) {
    std::vector<long long> kind(p.row_kind.begin(), p.row_kind.end()), ref(p.row_ref.begin(), p.row_ref.end()), bits(p.row_bits.begin(), p.row_bits.end());
    std::vector<long long> live, next, label, neg;
    for (const SessionSlot& sl : p.slot) { live.push_back(sl.live); next.push_back(sl.live ? sl.next : -1); label.push_back(sl.label_row); neg.push_back(sl.neg_row); }
    std::printf(", \"live\": %d, \"rows_used\": %d, \"steps\": %lld, \"rows_cond\": %lld, \"rows_uncond\": %lld, \"sig_rows\": %zu, \"solo_rows_cond\": %lld, \"solo_rows_uncond\": %lld",
                p.live, p.rows_used, (long long)p.steps, (long long)p.rows_cond, (long long)p.rows_uncond, p.sig_row.size(), solo_cond, solo_uncond);
    print_ints("row_kind", kind); print_ints("row_ref", ref); print_ints("row_bits", bits);
    print_ints("slot_live", live); print_ints("slot_next", next); print_ints("slot_label", label); print_ints("slot_neg", neg);
    std::vector<long long> sig;
    for (const SessionSlot& sl : p.slot) { sig.push_back(-1); for (int r : sl.sig_row) sig.push_back(r); }
    print_ints("slot_sig", sig);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s SCRIPT.txt\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    SessionPlan plan;
    SessionStep st;
    SessionAdmit ad;
    std::vector<Solo> solo;                  // per slot: the request in it, alone
    long long solo_cond = 0, solo_uncond = 0;
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "open") {
            int slots, rows, skip, max_batch;
            in >> slots >> rows >> skip >> max_batch;
            const SampleRefusal bad = session_open_check(slots, rows, max_batch);
            std::printf("{\"op\": \"open\", \"check\": [%d, %s]}\n", bad.code, quoted(bad.msg).c_str());
            if (!bad) { plan.open(slots, rows, skip != 0); solo.assign((size_t)slots, Solo()); solo_cond = solo_uncond = 0; }
        } else if (op == "admit") {
            tld_session_request r{};
            std::string g;
            int has_neg_label;
            in >> r.n_levels >> g >> r.has_negative >> has_neg_label >> r.reserved;
            r.class_guidance = from_bits((uint32_t)std::strtoul(g.c_str(), nullptr, 16));
            std::vector<float> coeffs, guidance, noise_coeff;
            std::vector<uint64_t> keys;
            r.coeffs = read_floats(in, "C", coeffs) ? coeffs.data() : nullptr;
            r.guidance = read_floats(in, "G", guidance) ? guidance.data() : nullptr;
            r.noise_coeff = read_floats(in, "E", noise_coeff) ? noise_coeff.data() : nullptr;
            std::string t; long n_keys;
            in >> t >> n_keys;
            for (long k = 0; k < n_keys; ++k) { std::string h; in >> h; keys.push_back(std::strtoull(h.c_str(), nullptr, 16)); }
            r.noise_key = n_keys >= 0 ? keys.data() : nullptr;
            static const float some_label = 0.0f;      // (the plan never reads device pointers: any non-null value stands for one)
            r.neg_label = has_neg_label ? &some_label : nullptr;
            if (!in) { std::fprintf(stderr, "admit: a short line\n"); return 2; }
            const SampleRefusal bad = session_request_check(&r);
            std::printf("{\"op\": \"admit\", \"check\": [%d, %s]", bad.code, quoted(bad.msg).c_str());
            if (!bad) {
                const SampleRefusal full = session_admit(plan, r, ad);
                std::printf(", \"admit\": [%d, %s], \"slot\": %d, \"label_row\": %d, \"neg_row\": %d", full.code, quoted(full.msg).c_str(), ad.slot, ad.label_row, ad.neg_row);
                std::vector<long long> ns;
                for (const auto& q : ad.new_sigma) { ns.push_back(q.first); ns.push_back(session_bits(q.second)); }
                print_ints("new_sigma", ns);
                if (!full && ad.slot >= 0) {
                    Solo& s = solo[(size_t)ad.slot];
                    make_solo(r, plan.skip, s);
                    std::printf(", \"solo_planned\": %d", (int)s.ok);
                    if (s.ok) { solo_cond += s.plan.rows_cond; solo_uncond += s.plan.rows_uncond; }
                }
                print_state(plan, solo_cond, solo_uncond);
            }
            std::printf("}\n");
        } else if (op == "step") {
            std::vector<std::pair<int, int>> at;     // (slot, forward) of the live requests, before the step moves them
            for (int s = 0; s < plan.slots; ++s) if (plan.slot[(size_t)s].live) at.emplace_back(s, plan.slot[(size_t)s].next);
            const size_t cap = plan.max_up_bytes();
            unsigned char* buf = static_cast<unsigned char*>(std::malloc(cap ? cap : 1));       // exactly: a write past the end is the sanitizer's
            memset(buf, 0xCD, cap);
            session_step(plan, st, buf);
            std::printf("{\"op\": \"step\", \"Bi\": %d, \"U\": %d, \"mb\": %d, \"noise\": %d, \"noise_off\": %zu, \"ints_off\": %zu, \"up_bytes\": %zu", st.Bi, st.U, st.mb,
                        (int)st.noise, st.noise_off, st.ints_off, st.up_bytes);
            print_ints("finished", st.finished);
            std::printf(", \"bytes\": \"");
            for (size_t k = 0; k < st.up_bytes; ++k) std::printf("%02x", buf[k]);
            std::printf("\"");
            bool tail = st.up_bytes <= cap;
            for (size_t k = st.up_bytes; k < cap; ++k) tail = tail && buf[k] == 0xCD;
            bool same = (int)at.size() == st.Bi;
            const SamplerStepRow* tab = reinterpret_cast<const SamplerStepRow*>(buf);
            const SamplerNoiseRow* nt = reinterpret_cast<const SamplerNoiseRow*>(buf + st.noise_off);
            for (int b = 0; same && b < st.Bi; ++b) {
                const Solo& s = solo[(size_t)at[(size_t)b].first];
                const int i = at[(size_t)b].second;
                if (!s.ok) { same = false; break; }
                const SamplerStepRow& mine = tab[b];
                const SamplerStepRow& alone = reinterpret_cast<const SamplerStepRow*>(s.bytes.data())[i];
                same = same && memcmp(&mine, &alone, 7 * sizeof(float)) == 0 && (mine.final_step & 1) == (alone.final_step & 1);
                // the unconditional sample: a solo call without slots runs one at every forward
                same = same && ((mine.final_step >> 1) != 0) == (s.plan.slots ? (alone.final_step >> 1) != 0 : true);
                if (st.noise) {
                    const SamplerNoiseRow& e = nt[b];
                    same = same && e.reserved == (uint32_t)i;
                    if (s.plan.noise) {
                        const SamplerNoiseRow& ea = reinterpret_cast<const SamplerNoiseRow*>(s.bytes.data() + s.plan.noise_off)[i];
                        same = same && memcmp(&e.e, &ea.e, 4) == 0 && e.key_lo == ea.key_lo && e.key_hi == ea.key_hi;
                    } else {
                        same = same && e.e == 0.0f;
                    }
                } else {
                    same = same && !s.plan.noise;
                }
            }
            std::printf(", \"tail\": %d, \"solo\": %d", (int)tail, (int)same);
            print_state(plan, solo_cond, solo_uncond);
            std::printf("}\n");
            std::free(buf);
        } else {
            std::fprintf(stderr, "unknown command %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}
