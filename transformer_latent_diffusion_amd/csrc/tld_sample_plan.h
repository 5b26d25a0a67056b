// tld_sample_plan.h -- what one sampler call tells the kernels (tld_engine.hip: the six tld_sample* entries): a pure function
// from the call as an entry receives it to the argument refusals, the flavour of the step, the walk over the steps and the bytes of the one staged
// upload.  No HIP in this file: tests/host/sample_plan_main.cpp compiles it on its own and tests/sample_plan_ref.py restates it in numpy.
//
// The entries: check (sample_call_check), the null-engine and `finalized` tests, plan (sample_plan, which refuses what needs the engine's max_batch
// or the plan's own counts), then run_sampler fills the pinned buffer (sample_plan_fill) and launches one loop over plan.steps.
//
// The flavour rule (`table`: a guidance table is present):
//   entry        table   slots  noise  shape  skip           batch check
//   uniform        -       -      -      -      -            2 B <= max_batch
//   requests       -       -      -      -      -            2 B <= max_batch
//   guided        yes     yes     -      -    engine's       B_i + U_i <= max_batch at every step
//   stochastic    yes     yes    yes     -    engine's       B_i + U_i <= max_batch at every step
//   stochastic    no      yes    yes     -      -            2 B <= max_batch
//   shaped        yes     yes    yes    yes   engine's       B_i + U_i <= max_batch at every step
//   shaped        no      yes    yes    yes     -            2 B <= max_batch
// Without a table a slots call takes the record's class_guidance at every forward; a shaped call without noise_coeff runs `noise` on all-zero rows.
//
// The upload, in bytes from the start of the staging buffer (tabB = B with a row per request, 1 for the uniform entries):
//   0           SamplerStepRow [n_max][tabB]
//   mix_off     float [tabB]                                    the start mixes
//   rows_off    int, per step [noise rows mb | label rows mb (| source rows mb: slots)]     mb = B_i + U_i model samples; steps[i].rows_off counts ints
//   noise_off   SamplerNoiseRow [n_max][tabB]                   noise only; 16-byte aligned, the bytes of the gap are not written
//   shape_off   GuidanceShape [tabB]                            shape only
//   up_bytes    float [Tn]                                      the sigmas, behind the upload: they travel in a copy of their own
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tld_hip.h"      // tld_sample_request, TLD_ERR_*
#include "tld_guidance_shape.h"
#include "tld_sampler_rows.h"

namespace tld {

// the most conditioning token rows one tld_sample_requests call may need (distinct sigmas + label rows): at the 100 M width a row of cond.wq + cond.kv is
// about 0.52 MB, so the grow-only tables stay near 0.5 GiB
constexpr int kMaxRequestCondRows = 1024;

enum SampleEntry { SE_UNIFORM, SE_REQUESTS, SE_GUIDED, SE_STOCHASTIC, SE_SHAPED };      // tld_sample / tld_sample_from, then the four tld_sample_requests*

// The call as its entry received it; every array is on the HOST.  Request b is requests[b * stride] with the coefficient table
// coeffs + b * stride * n_max * 6: stride 1 for the tld_sample_requests* entries, 0 for the uniform ones (one record and one table for the whole batch).
struct SampleCall {
    SampleEntry entry;
    int B, n_max, stride;
    const tld_sample_request* requests;
    const float* coeffs;                 // [B or 1][n_max][6]: (sigma, a, b, c, c1, c2) per level
    const float* guidance;               // [B][n_max] or null: the guidance of request b's forward i instead of its record's
    const float* noise_coeff;            // [B][n_max] or null: e of request b's forward i
    const uint64_t* noise_keys;          // [B] or null
    const float* shape;                  // [B][4] or null: (eta_par, norm_r, beta, phi) of request b
    bool has_mask, has_init, has_neg_labels;      // which optional device operands came with the call
    bool guidance_skip; int max_batch;   // the engine's: read by sample_plan only, so an entry fills them after its null-engine test

    const tld_sample_request& req(int b) const { return requests[(size_t)b * stride]; }
    float g(int b, int i) const { return guidance ? guidance[(size_t)b * n_max + i] : req(b).class_guidance; }
    GuidanceShape shape_row(int b) const { return GuidanceShape{shape[4 * b], shape[4 * b + 1], shape[4 * b + 2], shape[4 * b + 3]}; }
};

struct SampleRefusal {
    int code = TLD_OK;
    std::string msg;                     // empty: fine
    explicit operator bool() const { return code != TLD_OK; }
};

inline SampleRefusal sample_refuse(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return SampleRefusal{code, buf};
}

// The argument refusals that need neither the engine nor the device, in the entries' order.  The uniform entries have tested their pointers already;
// the tld_sample_requests* entries test theirs (engine, noise, labels, out_latent) after this.
inline SampleRefusal sample_call_check(const SampleCall& c) {
    const int INV = TLD_ERR_INVALID;
    if (c.entry == SE_UNIFORM) {
        const float mix = c.requests[0].start_mix;
        if (!(mix > 0.0f && mix <= 1.0f)) return sample_refuse(INV, "start_mix %g outside (0, 1]", (double)mix);
        if (!c.has_init && (c.has_mask || mix < 1.0f)) return sample_refuse(INV, "init_latent is required with a mask or with start_mix < 1");
        return {};
    }
    if (c.entry == SE_SHAPED) {
        if (!c.shape) return sample_refuse(INV, "null argument: shape");
        if ((c.noise_coeff == nullptr) != (c.noise_keys == nullptr)) return sample_refuse(INV, "noise_coeff and noise_keys come together (both NULL: no noise)");
        if (c.B <= 0 || c.n_max <= 0) return sample_refuse(INV, "need positive sizes (batch %d, n_max %d)", c.B, c.n_max);
    }
    const int B = c.B, n_max = c.n_max;
    if (!c.requests || !c.coeffs || B <= 0 || (c.entry == SE_GUIDED && !c.guidance)) return sample_refuse(INV, "null argument");
    if (c.entry == SE_STOCHASTIC && !c.noise_coeff) return sample_refuse(INV, "null argument: noise_coeff");
    if (c.entry == SE_STOCHASTIC && !c.noise_keys) return sample_refuse(INV, "null argument: noise_keys");
    for (int b = 0; c.shape && b < B; ++b) {
        const GuidanceShape h = c.shape_row(b);
        if (const char* bad = guidance_shape_invalid(h))
            return sample_refuse(INV, "request %d: shape (%g, %g, %g, %g): bad %s", b, (double)h.eta_par, (double)h.norm_r, (double)h.beta, (double)h.phi, bad);
    }
    if (c.has_mask && !c.has_init) return sample_refuse(INV, "init_latent is required with a mask");
    for (int b = 0; b < B; ++b) {
        const tld_sample_request& r = c.requests[b];
        if (r.n_levels < 2) return sample_refuse(INV, "request %d: need at least two noise levels (have %d)", b, r.n_levels);
        if (r.n_levels > n_max) return sample_refuse(INV, "request %d: %d levels beside a coefficient table of n_max = %d", b, r.n_levels, n_max);
        if (b > 0 && r.n_levels > c.requests[b - 1].n_levels)
            return sample_refuse(INV, "request %d has %d levels after request %d with %d: the records must be ordered by non-increasing n_levels", b,
                                 r.n_levels, b - 1, c.requests[b - 1].n_levels);
        if (!(r.start_mix > 0.0f && r.start_mix <= 1.0f)) return sample_refuse(INV, "request %d: start_mix %g outside (0, 1]", b, (double)r.start_mix);
        if (!c.guidance && !std::isfinite(r.class_guidance)) return sample_refuse(INV, "request %d: class_guidance is not finite", b);
        for (int i = 0; c.guidance && i < r.n_levels; ++i)
            if (!std::isfinite(c.guidance[(size_t)b * n_max + i])) return sample_refuse(INV, "request %d: guidance of forward %d is not finite", b, i);
        if (r.start_mix < 1.0f && !c.has_init) return sample_refuse(INV, "request %d: init_latent is required with start_mix < 1", b);
        if (r.has_negative && !c.has_neg_labels) return sample_refuse(INV, "request %d: has_negative without neg_labels", b);
        for (int i = 0; c.noise_coeff && i < r.n_levels; ++i) {
            const float en = c.noise_coeff[(size_t)b * n_max + i];
            if (!(std::isfinite(en) && en >= 0.0f))
                return sample_refuse(INV, "request %d: noise_coeff of forward %d is %g: expected finite and >= 0", b, i, (double)en);
            if (i == r.n_levels - 1 && en != 0.0f)
                return sample_refuse(INV, "request %d: noise_coeff of its final forward %d is %g: the final prediction takes no noise, expected 0", b, i, (double)en);
        }
    }
    if (c.requests[0].n_levels != n_max) return sample_refuse(INV, "n_max = %d, but the longest request has %d levels", n_max, c.requests[0].n_levels);
    return {};
}

// Step i of the call: the model runs on the Bi requests still running (a prefix: the records are ordered by non-increasing n_levels) and on U
// unconditional samples, mb = Bi + U in all
struct SampleStep {
    int Bi, U, mb;
    size_t rows_off;                     // where the step's int tables start, in ints behind SamplePlan::rows_off
    bool stats;                          // a running request is shaped, has an unconditional sample and is guided at other than 1.0f: the statistics kernel runs
};

struct SamplePlan {
    // the flavour of the step kernel.  slots: a request has an unconditional sample only where slot >= 0, and the step carries a third int table;
    // noise: the second device table; shape: the third; skip: a forward guided at exactly 1.0f gets no slot
    bool slots, noise, shape, skip;
    int B, n_max, stride, tabB;
    int per;                             // int tables per step: noise rows, label rows (, source rows), one entry per model sample
    std::vector<SampleStep> steps;       // [n_max]
    std::vector<int> slot;               // [n_max][B]: the place of running request b's unconditional sample among the step's, or -1: none (x0 = cond itself)
    // conditioning rows: Tn noise rows, B label rows, the zero row, one row per negative label
    int Tn, n_neg, T;
    std::vector<float> sig;              // [Tn] the distinct sigmas in order of first use (by bit pattern); the uniform entries: level t itself
    std::vector<int> noise_idx;          // [n_max][B]: the row of request b's sigma at step i
    int64_t rows_cond, rows_uncond;      // model samples of the whole call (tld_engine_sample_rows)
    bool any_mix, any_shape, any_mom;    // a start_mix < 1; a step with `stats`; ... of a request with beta != 0
    size_t mix_off, rows_off, noise_off, shape_off, up_bytes;       // the upload (see the head of this file)
    size_t stage_bytes;                  // up_bytes + the sigma block
};

// The plan of a call that passed sample_call_check.  Refuses (before anything is planned, or at the first step that does not fit) what needs the
// engine's max_batch, and the conditioning row cap.  `p` may be reused from call to call: a steady state allocates nothing but the sigma map.
inline SampleRefusal sample_plan(const SampleCall& c, SamplePlan& p) {
    const int INV = TLD_ERR_INVALID;
    const int B = c.B, n_max = c.n_max;
    const bool table = c.guidance != nullptr;
    if (c.entry == SE_UNIFORM) {
        if (B <= 0 || 2 * B > c.max_batch) return sample_refuse(INV, "sampler batch %d needs max_batch >= %d (have %d)", B, 2 * B, c.max_batch);
        if (n_max < 2) return sample_refuse(INV, "need at least two noise levels");
    } else if (!table && 2 * B > c.max_batch) {
        return sample_refuse(INV, "sampler batch %d needs max_batch >= %d (have %d)", B, 2 * B, c.max_batch);
    }
    p.slots = c.entry == SE_GUIDED || c.entry == SE_STOCHASTIC || c.entry == SE_SHAPED;
    p.noise = c.entry == SE_STOCHASTIC || c.entry == SE_SHAPED;
    p.shape = c.entry == SE_SHAPED;
    p.skip = p.slots && table && c.guidance_skip;
    p.B = B; p.n_max = n_max; p.stride = c.stride; p.tabB = c.stride ? B : 1;
    p.per = p.slots ? 3 : 2;

    // ---- the one walk over the steps
    p.steps.resize((size_t)n_max);
    p.slot.resize((size_t)n_max * B);
    p.rows_cond = p.rows_uncond = 0;
    p.any_shape = p.any_mom = false;
    size_t row_ints = 0;
    for (int i = 0, Bi = B; i < n_max; ++i) {
        while (c.req(Bi - 1).n_levels <= i) --Bi;
        SampleStep& st = p.steps[(size_t)i];
        int* slot = &p.slot[(size_t)i * B];
        int U = 0;
        st.stats = false;
        for (int b = 0; b < Bi; ++b) {
            slot[b] = (!p.skip || c.g(b, i) != 1.0f) ? U++ : -1;
            if (!p.shape || slot[b] < 0 || c.g(b, i) == 1.0f) continue;
            const GuidanceShape h = c.shape_row(b);
            if (!h.neutral()) { st.stats = true; p.any_shape = true; p.any_mom |= h.beta != 0.0f; }
        }
        st.Bi = Bi; st.U = U; st.mb = Bi + U; st.rows_off = row_ints;
        if (table && st.mb > c.max_batch)
            return sample_refuse(INV, "step %d runs %d requests and %d unconditional samples: needs max_batch >= %d (have %d)", i, Bi, U, st.mb, c.max_batch);
        row_ints += (size_t)p.per * st.mb;
        p.rows_cond += Bi; p.rows_uncond += U;
    }

    // ---- the distinct float32 sigmas of every (request, step): requests that share a schedule share conditioning rows
    p.sig.clear();
    p.noise_idx.assign((size_t)n_max * B, 0);
    p.n_neg = 0;
    p.any_mix = false;
    for (int b = 0; b < B; ++b) { p.n_neg += c.req(b).has_negative ? 1 : 0; p.any_mix |= c.req(b).start_mix < 1.0f; }
    if (!c.stride) {                     // one table for the whole batch: row i is level i
        for (int i = 0; i < n_max; ++i) {
            p.sig.push_back(c.coeffs[(size_t)i * 6]);
            for (int b = 0; b < B; ++b) p.noise_idx[(size_t)i * B + b] = i;
        }
    } else {
        std::unordered_map<uint32_t, int> sig_row;            // by bit pattern
        for (int i = 0; i < n_max; ++i)
            for (int b = 0; b < p.steps[(size_t)i].Bi; ++b) {
                const float sg = c.coeffs[((size_t)b * n_max + i) * 6 + 0];
                uint32_t bits; memcpy(&bits, &sg, 4);
                auto it = sig_row.find(bits);
                if (it == sig_row.end()) { it = sig_row.emplace(bits, (int)p.sig.size()).first; p.sig.push_back(sg); }
                p.noise_idx[(size_t)i * B + b] = it->second;
            }
    }
    p.Tn = (int)p.sig.size();
    p.T = p.Tn + B + 1 + p.n_neg;
    if (c.stride && p.T > kMaxRequestCondRows)
        return sample_refuse(INV, "the call needs %d conditioning rows (%d distinct noise levels + %d labels + 1 + %d negative labels): at most %d", p.T, p.Tn,
                             B, p.n_neg, kMaxRequestCondRows);

    // ---- the upload
    const size_t cells = (size_t)n_max * p.tabB;
    p.mix_off = cells * sizeof(SamplerStepRow);
    p.rows_off = p.mix_off + (size_t)p.tabB * sizeof(float);
    const size_t rows_end = p.rows_off + row_ints * sizeof(int);
    p.noise_off = (rows_end + 15) & ~(size_t)15;
    p.shape_off = p.noise_off + cells * sizeof(SamplerNoiseRow);
    p.up_bytes = p.shape ? p.shape_off + (size_t)p.tabB * sizeof(GuidanceShape) : p.noise ? p.shape_off : rows_end;
    p.stage_bytes = p.up_bytes + (size_t)p.Tn * sizeof(float);
    return {};
}

// The upload and the sigma block into `staging` (p.stage_bytes, 16-byte aligned), from the call the plan was made of
inline void sample_plan_fill(const SamplePlan& p, const SampleCall& c, void* staging) {
    char* base = static_cast<char*>(staging);
    const int B = p.B, n_max = p.n_max, tabB = p.tabB, Tn = p.Tn;
    SamplerStepRow* tab = reinterpret_cast<SamplerStepRow*>(base);
    float* mix = reinterpret_cast<float*>(base + p.mix_off);
    for (int b = 0; b < tabB; ++b) {
        const tld_sample_request& r = c.req(b);
        const float* co = c.coeffs + (size_t)b * n_max * 6;
        mix[b] = r.start_mix;
        for (int i = 0; i < n_max; ++i, co += 6) {
            SamplerStepRow& u = tab[(size_t)i * tabB + b];
            if (i >= r.n_levels) { u = SamplerStepRow{}; continue; }
            u.g = c.g(b, i); u.a = co[1]; u.b = co[2]; u.c = co[3]; u.c1 = co[4]; u.c2 = co[5];
            u.s_next = (i + 1 < r.n_levels) ? co[6] : 0.0f;   // sigma of the request's next row
            u.final_step = (i == r.n_levels - 1) ? 1 : 0;
        }
    }
    for (int i = 0; i < n_max; ++i) {
        const SampleStep& st = p.steps[(size_t)i];
        const int Bi = st.Bi, mb = st.mb;
        int *nr = reinterpret_cast<int*>(base + p.rows_off) + st.rows_off, *lr = nr + mb, *sr = lr + mb;       // (sr: slots only)
        for (int b = 0, k = 0; b < Bi; ++b) {
            const int neg = c.req(b).has_negative ? Tn + B + 1 + k++ : Tn + B;      // the unconditional label: the zero row, or the request's own negative
            const int sl = p.slot[(size_t)i * B + b];
            nr[b] = p.noise_idx[(size_t)i * B + b];
            lr[b] = Tn + b;
            if (p.slots) { sr[b] = b; tab[(size_t)i * tabB + b].final_step |= (sl + 1) << 1; }
            if (sl < 0) continue;
            nr[Bi + sl] = nr[b];
            lr[Bi + sl] = neg;
            if (p.slots) sr[Bi + sl] = b;
        }
    }
    if (p.noise) {                       // (no noise_coeff: the shaped entry without noise, all-zero rows -- nothing is drawn, nothing added)
        SamplerNoiseRow* nt = reinterpret_cast<SamplerNoiseRow*>(base + p.noise_off);
        for (int b = 0; b < tabB; ++b) {
            const uint64_t key = c.noise_keys ? c.noise_keys[b] : 0;
            for (int i = 0; i < n_max; ++i) {
                const bool on = c.noise_coeff && i < c.req(b).n_levels - 1;         // (the final forward adds none: its entry was checked to be 0)
                nt[(size_t)i * tabB + b] = SamplerNoiseRow{on ? c.noise_coeff[(size_t)b * n_max + i] : 0.0f, (uint32_t)key, (uint32_t)(key >> 32), 0u};
            }
        }
    }
    if (p.shape) {
        GuidanceShape* sh = reinterpret_cast<GuidanceShape*>(base + p.shape_off);
        for (int b = 0; b < tabB; ++b) sh[b] = c.shape_row(b);
    }
    memcpy(base + p.up_bytes, p.sig.data(), (size_t)Tn * sizeof(float));
}

}  // namespace tld
