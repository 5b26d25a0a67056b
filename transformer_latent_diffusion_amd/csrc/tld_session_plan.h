// tld_session_plan.h -- the host side of a sampler session (tld_engine.hip: the tld_session_* entries): which request sits in
// which slot, which conditioning rows it owns, and the bytes of the one staged upload of every step.  No HIP in this file:
// tests/host/session_plan_main.cpp compiles it on its own and tests/session_plan_ref.py restates it in numpy.
//
// A session holds `slots` slots of per-request state and a conditioning-row table of `cond_rows` rows.  Row 0 is the zero label.  A live request owns
// one label row, one more with a negative label, and a reference on the row of every distinct float32 sigma (by bit pattern) of its table: requests on
// the same schedule share those rows.  Rows are handed out lowest-free-first.  A request holds its rows from admit until the step of its final forward.
//
// One step takes the live requests in ascending slot order as b = 0 .. Bi - 1, each at its own forward index, and emits (session_step):
//   0           SamplerStepRow  [Bi]      the row sample_plan_fill writes for the request alone at that forward; final_step = final | (uslot + 1) << 1
//   noise_off   SamplerNoiseRow [Bi]      only while a live request is stochastic; `reserved` holds the request's own forward index
//   ints_off    int req_slot [Bi] | noise row [mb] | label row [mb] | source request [mb] | embed slot [mb]          mb = Bi + U model samples
//   up_bytes
// The unconditional sample of request b is model sample Bi + uslot; a request with a guidance table and a forward guided at exactly 1.0f has none
// when the engine's guidance_skip is on (the rule of the guided entry, per request).
#pragma once

#include <algorithm>
#include <utility>

#include "tld_sample_plan.h"

namespace tld {

// What admit keeps of a request: every array of tld_session_request is copied, so the caller's may go after the call
struct SessionRequest {
    int n_levels = 0;
    float class_guidance = 0.0f;
    bool has_negative = false, has_table = false, has_noise = false;
    uint64_t key = 0;
    std::vector<float> coeffs;           // [n_levels][6]
    std::vector<float> guidance;         // [n_levels] with has_table
    std::vector<float> noise_coeff;      // [n_levels] with has_noise
    float g(int i) const { return has_table ? guidance[(size_t)i] : class_guidance; }
};

struct SessionSlot {
    bool live = false;
    int next = 0;                        // index of the request's next forward
    int label_row = -1, neg_row = -1;    // neg_row < 0: the zero row
    std::vector<int> sig_row;            // [n_levels]: the row of the sigma of forward i
    SessionRequest rq;
};

enum SessionRowKind : uint8_t { SR_FREE = 0, SR_ZERO, SR_LABEL, SR_SIGMA };

struct SessionAdmit {
    int slot = -1;                                   // -1: no room now (no free slot, or too few free rows)
    std::vector<std::pair<int, float>> new_sigma;    // the rows to compute: (row, sigma), in order of first use
    int label_row = -1, neg_row = -1;                // the label rows to fill
};

struct SessionStep {
    int Bi = 0, U = 0, mb = 0;
    bool noise = false;
    size_t noise_off = 0, ints_off = 0, up_bytes = 0;
    std::vector<int> finished;           // the slots whose request ran its final forward in this step, ascending
};

struct SessionPlan {
    int slots = 0, cond_rows = 0;
    bool skip = true;                    // the engine's guidance_skip
    std::vector<SessionSlot> slot;
    std::vector<uint8_t> row_kind;       // [cond_rows]
    std::vector<int> row_ref;            // [cond_rows]: live requests that hold the row
    std::vector<uint32_t> row_bits;      // [cond_rows]: SR_SIGMA: the sigma's bit pattern
    std::unordered_map<uint32_t, int> sig_row;
    int live = 0, rows_used = 0;
    int64_t steps = 0, rows_cond = 0, rows_uncond = 0;

    void open(int slots_, int cond_rows_, bool skip_) {
        *this = SessionPlan();
        slots = slots_; cond_rows = cond_rows_; skip = skip_;
        slot.resize((size_t)slots);
        row_kind.assign((size_t)cond_rows, SR_FREE); row_ref.assign((size_t)cond_rows, 0); row_bits.assign((size_t)cond_rows, 0u);
        row_kind[0] = SR_ZERO; rows_used = 1;
    }
    // the largest upload a step of this session can make
    size_t max_up_bytes() const { return (size_t)slots * (sizeof(SamplerStepRow) + sizeof(SamplerNoiseRow) + sizeof(int)) + (size_t)8 * slots * sizeof(int); }
};

inline uint32_t session_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the sizes a session may be opened with, beside the engine's max_batch (every step of S slots fits 2 S model samples)
inline SampleRefusal session_open_check(int slots, int cond_rows, int max_batch) {
    const int INV = TLD_ERR_INVALID;
    if (slots < 1) return sample_refuse(INV, "a session needs at least one slot (have %d)", slots);
    if (2 * slots > max_batch) return sample_refuse(INV, "a session of %d slots needs max_batch >= %d (have %d)", slots, 2 * slots, max_batch);
    if (cond_rows < 3 || cond_rows > kMaxRequestCondRows)
        return sample_refuse(INV, "cond_rows = %d: a session takes 3 .. %d conditioning rows", cond_rows, kMaxRequestCondRows);
    return {};
}

// The refusals of a request that need neither the session nor the device, in sample_call_check's wording where the rule is the same
inline SampleRefusal session_request_check(const tld_session_request* r) {
    const int INV = TLD_ERR_INVALID;
    if (!r || !r->coeffs) return sample_refuse(INV, "null argument");
    if (r->reserved != 0) return sample_refuse(INV, "request: reserved = %d: expected 0", r->reserved);
    if ((r->noise_coeff == nullptr) != (r->noise_key == nullptr)) return sample_refuse(INV, "noise_coeff and noise_key come together (both NULL: no noise)");
    if (r->n_levels < 2) return sample_refuse(INV, "request: need at least two noise levels (have %d)", r->n_levels);
    if (!r->guidance && !std::isfinite(r->class_guidance)) return sample_refuse(INV, "request: class_guidance is not finite");
    for (int i = 0; r->guidance && i < r->n_levels; ++i)
        if (!std::isfinite(r->guidance[i])) return sample_refuse(INV, "request: guidance of forward %d is not finite", i);
    if (r->has_negative && !r->neg_label) return sample_refuse(INV, "request: has_negative without neg_label");
    for (int i = 0; r->noise_coeff && i < r->n_levels; ++i) {
        const float en = r->noise_coeff[i];
        if (!(std::isfinite(en) && en >= 0.0f)) return sample_refuse(INV, "request: noise_coeff of forward %d is %g: expected finite and >= 0", i, (double)en);
        if (i == r->n_levels - 1 && en != 0.0f)
            return sample_refuse(INV, "request: noise_coeff of its final forward %d is %g: the final prediction takes no noise, expected 0", i, (double)en);
    }
    return {};
}

// A request that passed session_request_check into the session.  TLD_ERR_INVALID: it could never fit.  out.slot == -1 with no refusal: no room now.
inline SampleRefusal session_admit(SessionPlan& p, const tld_session_request& r, SessionAdmit& out) {
    out = SessionAdmit();
    const int n = r.n_levels;
    // the distinct sigmas in order of first use, and which of them have no row yet
    std::vector<uint32_t> distinct;
    for (int i = 0; i < n; ++i) {
        const uint32_t bits = session_bits(r.coeffs[(size_t)i * 6]);
        if (std::find(distinct.begin(), distinct.end(), bits) == distinct.end()) distinct.push_back(bits);
    }
    const int own = (int)distinct.size() + 1 + (r.has_negative ? 1 : 0);
    if (own > p.cond_rows - 1)
        return sample_refuse(TLD_ERR_INVALID, "the request needs %d conditioning rows (%d distinct noise levels + 1 label + %d negative label): the session has %d beside the zero row",
                             own, (int)distinct.size(), r.has_negative ? 1 : 0, p.cond_rows - 1);
    int fresh = 1 + (r.has_negative ? 1 : 0);
    for (uint32_t bits : distinct) fresh += p.sig_row.count(bits) ? 0 : 1;
    int s = 0;
    while (s < p.slots && p.slot[(size_t)s].live) ++s;
    if (s == p.slots || fresh > p.cond_rows - p.rows_used) return {};      // no room now

    int cursor = 0;
    auto take = [&](SessionRowKind kind) {
        while (p.row_kind[(size_t)cursor] != SR_FREE) ++cursor;
        p.row_kind[(size_t)cursor] = kind; p.row_ref[(size_t)cursor] = 1; ++p.rows_used;
        return cursor;
    };
    SessionSlot& sl = p.slot[(size_t)s];
    sl.live = true; sl.next = 0;
    SessionRequest& q = sl.rq;
    q.n_levels = n; q.class_guidance = r.class_guidance; q.has_negative = r.has_negative != 0;
    q.has_table = r.guidance != nullptr; q.has_noise = r.noise_coeff != nullptr; q.key = r.noise_key ? *r.noise_key : 0;
    q.coeffs.assign(r.coeffs, r.coeffs + (size_t)n * 6);
    q.guidance.clear(); q.noise_coeff.clear();
    if (q.has_table) q.guidance.assign(r.guidance, r.guidance + n);
    if (q.has_noise) q.noise_coeff.assign(r.noise_coeff, r.noise_coeff + n);
    for (uint32_t bits : distinct) {
        auto it = p.sig_row.find(bits);
        if (it != p.sig_row.end()) { ++p.row_ref[(size_t)it->second]; continue; }
        const int row = take(SR_SIGMA);
        p.row_bits[(size_t)row] = bits; p.sig_row.emplace(bits, row);
        float sg; memcpy(&sg, &bits, 4);
        out.new_sigma.emplace_back(row, sg);
    }
    sl.sig_row.resize((size_t)n);
    for (int i = 0; i < n; ++i) sl.sig_row[(size_t)i] = p.sig_row[session_bits(q.coeffs[(size_t)i * 6])];
    sl.label_row = take(SR_LABEL);
    sl.neg_row = q.has_negative ? take(SR_LABEL) : -1;
    out.slot = s; out.label_row = sl.label_row; out.neg_row = sl.neg_row;
    ++p.live;
    return {};
}

inline void session_release_row(SessionPlan& p, int row) {
    if (--p.row_ref[(size_t)row] > 0) return;
    if (p.row_kind[(size_t)row] == SR_SIGMA) p.sig_row.erase(p.row_bits[(size_t)row]);
    p.row_kind[(size_t)row] = SR_FREE; p.row_bits[(size_t)row] = 0; --p.rows_used;
}

// One step: the tables of every live request's next forward into `staging` (p.max_up_bytes(), 16-byte aligned), then the requests move on and the
// finished ones give their rows and slots back.  No live request: nothing is written and st.Bi == 0.
inline void session_step(SessionPlan& p, SessionStep& st, void* staging) {
    st.finished.clear();
    st.Bi = st.U = st.mb = 0; st.noise = false; st.noise_off = st.ints_off = st.up_bytes = 0;
    if (!p.live) return;
    int Bi = 0, U = 0;
    bool noise = false;
    for (const SessionSlot& sl : p.slot) {
        if (!sl.live) continue;
        ++Bi; noise |= sl.rq.has_noise;
        if (!(p.skip && sl.rq.has_table) || sl.rq.g(sl.next) != 1.0f) ++U;
    }
    const int mb = Bi + U;
    st.Bi = Bi; st.U = U; st.mb = mb; st.noise = noise;
    st.noise_off = (size_t)Bi * sizeof(SamplerStepRow);
    st.ints_off = st.noise_off + (noise ? (size_t)Bi * sizeof(SamplerNoiseRow) : 0);
    st.up_bytes = st.ints_off + ((size_t)Bi + (size_t)4 * mb) * sizeof(int);
    char* base = static_cast<char*>(staging);
    SamplerStepRow* tab = reinterpret_cast<SamplerStepRow*>(base);
    SamplerNoiseRow* nt = reinterpret_cast<SamplerNoiseRow*>(base + st.noise_off);
    int *rs = reinterpret_cast<int*>(base + st.ints_off), *nr = rs + Bi, *lr = nr + mb, *sr = lr + mb, *es = sr + mb;
    int b = 0, u = 0;
    for (int s = 0; s < p.slots; ++s) {
        SessionSlot& sl = p.slot[(size_t)s];
        if (!sl.live) continue;
        const SessionRequest& q = sl.rq;
        const int i = sl.next;
        const float* co = q.coeffs.data() + (size_t)i * 6;
        const bool final_step = i == q.n_levels - 1;
        const int us = (!(p.skip && q.has_table) || q.g(i) != 1.0f) ? u++ : -1;
        SamplerStepRow& row = tab[b];
        row.g = q.g(i); row.a = co[1]; row.b = co[2]; row.c = co[3]; row.c1 = co[4]; row.c2 = co[5];
        row.s_next = final_step ? 0.0f : co[6];
        row.final_step = (final_step ? 1 : 0) | (us + 1) << 1;
        if (noise) {
            const bool on = q.has_noise && !final_step;
            nt[b] = SamplerNoiseRow{on ? q.noise_coeff[(size_t)i] : 0.0f, (uint32_t)q.key, (uint32_t)(q.key >> 32), (uint32_t)i};
        }
        rs[b] = s;
        nr[b] = sl.sig_row[(size_t)i]; lr[b] = sl.label_row; sr[b] = b; es[b] = s;
        if (us >= 0) { nr[Bi + us] = nr[b]; lr[Bi + us] = sl.neg_row < 0 ? 0 : sl.neg_row; sr[Bi + us] = b; es[Bi + us] = s; }
        ++b;
        if (final_step) st.finished.push_back(s);
        ++sl.next;
    }
    p.rows_cond += Bi; p.rows_uncond += U; ++p.steps;
    for (int s : st.finished) {
        SessionSlot& sl = p.slot[(size_t)s];
        std::vector<int> rows(sl.sig_row);
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        for (int row : rows) session_release_row(p, row);
        session_release_row(p, sl.label_row);
        if (sl.neg_row >= 0) session_release_row(p, sl.neg_row);
        sl.live = false; sl.label_row = sl.neg_row = -1; sl.sig_row.clear();
        --p.live;
    }
}

}  // namespace tld
