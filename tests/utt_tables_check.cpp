// utt_tables_check.cpp -- summertts_amd/csrc/utt_tables.hpp as a stand-alone program: tests/test_utt_tables_cpu.py builds it under
// AddressSanitizer and UBSan.  The staging layout against the expressions Engine::run_setup spelled out by hand before the layout
// existed (restated here: they are the truth the device addresses must keep), UttTables assign -> view bit for bit from sources that
// are freed before the view is read, the "present" rules, and the same-batch check.  Prints "ok <layouts> <round trips>".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "utt_tables.hpp"

using namespace sts;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

// ---- the layout
static long check_layouts() {
    long cases = 0;
    for (size_t B : {1, 2, 3, 65})
        for (size_t Ttot : {B, B + 1, (size_t)257})
            for (size_t mix_ints : {(size_t)0, 3 * B + 1, 3 * B + 1 + 2 * 5 + 7})      // none; B empty entries; 5 terms and one 7-float vector
                for (int gain = 0; gain < 2; gain++)
                    for (int join = 0; join < 2; join++)
                        for (int plan_set = 0; plan_set < 2; plan_set++)
                            for (int forced = 0; forced < 2; forced++)
                                for (int pitch = 0; pitch < 2; pitch++) {
                                    if (plan_set && forced) continue;       // refused by the run: both are dropped
                                    if (pitch && join) continue;            // a joined run refuses a pitch plan
                                    const bool plan = plan_set || (pitch && !forced);
                                    const size_t gain_ints = gain ? Ttot + B : 0, join_ints = join ? B : 0, plan_ints = plan ? 2 * Ttot + B : 0;
                                    const StageLayout L(B, Ttot, mix_ints, gain_ints, join != 0, plan, forced != 0);
                                    // the parent's expressions, in 32-bit words from the block's base
                                    const size_t meta_ints = 9 * B + 8;
                                    const size_t ids = meta_ints + 5 * B;          // ls B, ns B, nsw B, seed B uint64
                                    CHECK(L.meta == 0 && L.ls == meta_ints && L.ns == meta_ints + B && L.nsw == meta_ints + 2 * B && L.seed == meta_ints + 3 * B);
                                    CHECK(L.ids == ids);
                                    if (mix_ints) CHECK(L.mix == ids + Ttot);
                                    if (gain) CHECK(L.gain_q == ids + Ttot + mix_ints && L.gain_h == ids + 2 * Ttot + mix_ints);
                                    if (join) CHECK(L.join_sil == ids + Ttot + mix_ints + gain_ints);
                                    if (plan) {
                                        CHECK(L.plan_rate == ids + Ttot + mix_ints + gain_ints + join_ints);
                                        CHECK(L.plan_fixed == ids + 2 * Ttot + mix_ints + gain_ints + join_ints);
                                        CHECK(L.plan_target == ids + 3 * Ttot + mix_ints + gain_ints + join_ints);
                                    }
                                    CHECK(L.forced == ids + Ttot + mix_ints + gain_ints + join_ints + plan_ints);
                                    if (forced) CHECK(L.forced == ids + Ttot + mix_ints + gain_ints + join_ints);      // the pinned side's p_forced
                                    CHECK(L.words == meta_ints + 5 * B + 2 * Ttot + mix_ints + gain_ints + join_ints + plan_ints);
                                    CHECK(L.copy_words == meta_ints + 5 * B + Ttot * (forced ? 2 : 1) + mix_ints + gain_ints + join_ints + plan_ints);
                                    // sections in order, back to back, an absent one empty; the copy drops exactly `forced`
                                    const size_t off[] = {L.meta, L.ls, L.ns, L.nsw, L.seed, L.ids, L.mix, L.gain_q, L.gain_h, L.join_sil, L.plan_rate, L.plan_fixed,
                                                          L.plan_target, L.forced, L.words};
                                    const size_t size[] = {meta_ints, B, B, B, 2 * B, Ttot, mix_ints, gain ? Ttot : 0, gain ? B : 0, join_ints, plan ? Ttot : 0,
                                                           plan ? Ttot : 0, plan ? B : 0, Ttot};
                                    for (int i = 0; i < 14; i++) CHECK(off[i + 1] == off[i] + size[i]);
                                    CHECK((256 + L.seed * 4) % 8 == 0);
                                    CHECK(L.copy_words == (forced ? L.words : L.words - Ttot));
                                    cases++;
                                }
    return cases;
}

// ---- UttTables: sources live in exact-size heap blocks, freed before the view is read
template <typename T> static T* heap(const std::vector<T>& v) {
    T* p = (T*)malloc(v.size() * sizeof(T));       // (never empty here)
    memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <typename T> static bool same_bits(const T* a, const std::vector<T>& b) { return a && memcmp(a, b.data(), b.size() * sizeof(T)) == 0; }

static void check_empty(const UttTables& u) {
    CHECK(!u.has_duration() && !u.has_mix() && !u.has_gain() && !u.has_pitch());
    const sts_dur_plan d = u.view_duration();
    CHECK(!d.rate && !d.fixed && d.target_frames == 0);
    const sts_speaker_mix m = u.view_mix();
    CHECK(m.k == 0 && !m.sid && !m.weight && !m.vector && m.vector_weight == 0.f && speaker_mix_empty(m));
    const sts_gain_plan g = u.view_gain();
    CHECK(!g.gain_db && g.ramp_ms == 0.f);
    CHECK(!u.view_pitch().cents);
}

static void round_trip(UttTables& u, int n, bool with_rate, bool with_fixed, int32_t target, int k, bool with_vector, int gin, bool with_gain, bool with_cents) {
    std::vector<float> rate(n), gain(n), weight(k), vec(gin);
    std::vector<int32_t> fixed(n), cents(n), sid(k);
    for (int i = 0; i < n; i++) {
        rate[i] = 1.f / 64.f + (float)(rnd() % 4096) / 64.f; fixed[i] = (int)(rnd() % 50) - 1;
        gain[i] = rnd() % 5 == 0 ? -INFINITY : -96.f + (float)(rnd() % 1200) / 10.f; cents[i] = (int)(rnd() % 1201) - 600;
    }
    if (with_gain && n > 0) gain[0] = -INFINITY;
    for (int i = 0; i < k; i++) { sid[i] = (int)(rnd() % 100); weight[i] = (float)(rnd() % 3200) / 100.f - 16.f; }
    for (int i = 0; i < gin; i++) vec[i] = (float)(rnd() % 2000) / 1000.f - 1.f;
    const float ramp = (float)(rnd() % 500) / 10.f, vw = (float)(rnd() % 3200) / 100.f - 16.f;
    float* h_rate = with_rate ? heap(rate) : nullptr; int32_t* h_fixed = with_fixed ? heap(fixed) : nullptr;
    float* h_gain = with_gain ? heap(gain) : nullptr; int32_t* h_cents = with_cents ? heap(cents) : nullptr;
    int32_t* h_sid = k ? heap(sid) : nullptr; float* h_weight = k ? heap(weight) : nullptr; float* h_vec = with_vector ? heap(vec) : nullptr;
    u.assign_duration(sts_dur_plan{h_rate, h_fixed, target}, n);
    u.assign_mix(sts_speaker_mix{k, h_sid, h_weight, h_vec, vw}, gin);
    u.assign_gain(sts_gain_plan{h_gain, ramp}, n);
    u.assign_pitch(sts_pitch_plan{h_cents}, n);
    free(h_rate); free(h_fixed); free(h_gain); free(h_cents); free(h_sid); free(h_weight); free(h_vec);
    // the "present" rules of the four kinds
    CHECK(u.has_duration() == (with_rate || with_fixed || target != 0));
    CHECK(u.has_mix() == (k != 0 || with_vector));
    CHECK(u.has_gain() == with_gain);
    CHECK(u.has_pitch() == with_cents);
    const sts_dur_plan d = u.view_duration();
    CHECK(with_rate ? same_bits(d.rate, rate) : !d.rate);
    CHECK(with_fixed ? same_bits(d.fixed, fixed) : !d.fixed);
    CHECK(d.target_frames == target);
    const sts_speaker_mix m = u.view_mix();
    CHECK(m.k == k && (k ? same_bits(m.sid, sid) && same_bits(m.weight, weight) : !m.sid && !m.weight));
    CHECK(with_vector ? same_bits(m.vector, vec) && memcmp(&m.vector_weight, &vw, 4) == 0 : !m.vector && m.vector_weight == 0.f);
    CHECK(speaker_mix_empty(m) == !u.has_mix());
    const sts_gain_plan g = u.view_gain();
    CHECK(with_gain ? same_bits(g.gain_db, gain) : !g.gain_db);
    CHECK(memcmp(&g.ramp_ms, &ramp, 4) == 0);
    const sts_pitch_plan p = u.view_pitch();
    CHECK(with_cents ? same_bits(p.cents, cents) : !p.cents);
    // no stale tail behind a shorter table: the copies are exactly as long as what was assigned
    CHECK(u.rate.size() == (with_rate ? (size_t)n : 0) && u.fixed.size() == (with_fixed ? (size_t)n : 0));
    CHECK(u.gain_db.size() == (with_gain ? (size_t)n : 0) && u.cents.size() == (with_cents ? (size_t)n : 0));
    CHECK(u.mix.sid.size() == (size_t)k && u.mix.weight.size() == (size_t)k && u.mix.vector.size() == (with_vector ? (size_t)gin : 0));
}

static long check_tables() {
    long trips = 0;
    UttTables fresh;
    check_empty(fresh);
    UttTables u;       // one object through every case: a long table, then a shorter one, then absent ones
    for (int n : {21, 5, 1, 9})
        for (int mask = 0; mask < 64; mask++) {
            const bool with_rate = mask & 1, with_fixed = mask & 2, with_gain = mask & 4, with_cents = mask & 8, with_vector = mask & 16;
            const int k = mask & 32 ? 1 + (int)(rnd() % 16) : 0;
            round_trip(u, n, with_rate, with_fixed, mask % 3 == 0 ? 40 + n : 0, k, with_vector, 7, with_gain, with_cents);
            trips++;
        }
    // the cases the definition names: rate with fixed absent, a mix of a vector alone, an entry that carries nothing
    round_trip(u, 6, true, false, 0, 0, true, 3, true, false); trips++;
    CHECK(u.has_duration() && u.has_mix() && u.has_gain() && !u.has_pitch());
    round_trip(u, 6, false, false, 0, 0, false, 3, false, false); trips++;
    CHECK(!u.has_duration() && !u.has_mix() && !u.has_gain() && !u.has_pitch());
    // (a gain entry without gains keeps its ramp: the run's table carries its h.  Everything else of it is the empty entry)
    u.assign_gain(sts_gain_plan{nullptr, 0.f}, 6);
    check_empty(u);
    return trips;
}

static void check_matches() {
    const std::vector<int32_t> set_n = {5, 21, 7, 9, 13};
    const int B = (int)set_n.size();
    std::vector<int32_t> n = set_n;
    CHECK(table_matches(set_n, B, n.data()));
    CHECK(!table_matches(set_n, B - 1, n.data()));
    n.push_back(4);
    CHECK(!table_matches(set_n, B + 1, n.data()));
    for (int at : {0, B / 2, B - 1}) {
        std::vector<int32_t> other = set_n;
        other[at] += 1;
        CHECK(!table_matches(set_n, B, other.data()));
    }
    CHECK(table_matches(std::vector<int32_t>(), 0, nullptr) && !table_matches(std::vector<int32_t>(), 1, n.data()));
    CHECK(other_batch_message("duration plan") == "the duration plan was set for another batch (B and every n[b] must match)");
    CHECK(other_batch_message("speaker mix", false) == "the speaker mix was set for another batch (B must match)");
}

int main() {
    const long layouts = check_layouts();
    const long trips = check_tables();
    check_matches();
    printf("ok %ld %ld\n", layouts, trips);
    return 0;
}
