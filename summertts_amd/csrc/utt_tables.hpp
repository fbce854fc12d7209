// utt_tables.hpp -- the tables a caller may give for the next call only (duration plan, speaker mix, gain plan, pitch plan), as plain C++:
// the owning host copy of ONE utterance's tables (a request of a pool, an utterance of a multi-device batch), the one same-batch check,
// its one message, and the layout of the staging block a run uploads them in.  No device code and no engine type: the tests compile
// this header alone.  A further kind of table touches three places: UttTables here, apply_utt_tables (engine.hip) and StageLayout below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/summertts_hip.h"

namespace sts {

inline bool speaker_mix_empty(const sts_speaker_mix& m) { return m.k == 0 && !m.vector; }
// host copy of one speaker mix entry
struct SpeakerMixCopy {
    std::vector<int32_t> sid; std::vector<float> weight, vector; float vector_weight = 0.f; bool has_vector = false;
    void assign(const sts_speaker_mix& m, int gin) {
        sid.assign(m.sid, m.sid + (m.k > 0 ? m.k : 0)); weight.assign(m.weight, m.weight + (m.k > 0 ? m.k : 0));
        has_vector = m.vector != nullptr; vector_weight = has_vector ? m.vector_weight : 0.f;
        if (has_vector) vector.assign(m.vector, m.vector + gin); else vector.clear();
    }
    sts_speaker_mix view() const {
        return sts_speaker_mix{(int32_t)sid.size(), sid.empty() ? nullptr : sid.data(), weight.empty() ? nullptr : weight.data(),
                               has_vector ? vector.data() : nullptr, vector_weight};
    }
};

// One utterance's optional tables.  assign_*(entry, n) copies an entry its validator accepted (n >= 1 phonemes: an empty array is an
// absent one); view_*() is the public struct pointing into the copy, valid until the next assign -- of a kind that was never assigned,
// the empty entry, which the engine synthesises as without, bit for bit.  has_*(): the entry carries something.
struct UttTables {
    std::vector<float> rate; std::vector<int32_t> fixed; int32_t target = 0;
    SpeakerMixCopy mix;
    std::vector<float> gain_db; float ramp_ms = 0.f;     // (ramp_ms also of an entry without gains: its h still travels in the run's table)
    std::vector<int32_t> cents;

    bool has_duration() const { return !rate.empty() || !fixed.empty() || target != 0; }
    bool has_mix() const { return !speaker_mix_empty(mix.view()); }
    bool has_gain() const { return !gain_db.empty(); }
    bool has_pitch() const { return !cents.empty(); }

    void assign_duration(const sts_dur_plan& p, int n) {
        rate.assign(p.rate, p.rate + (p.rate ? n : 0)); fixed.assign(p.fixed, p.fixed + (p.fixed ? n : 0)); target = p.target_frames;
    }
    void assign_mix(const sts_speaker_mix& m, int gin) { mix.assign(m, gin); }
    void assign_gain(const sts_gain_plan& p, int n) { gain_db.assign(p.gain_db, p.gain_db + (p.gain_db ? n : 0)); ramp_ms = p.ramp_ms; }
    void assign_pitch(const sts_pitch_plan& p, int n) { cents.assign(p.cents, p.cents + (p.cents ? n : 0)); }

    sts_dur_plan view_duration() const { return sts_dur_plan{rate.empty() ? nullptr : rate.data(), fixed.empty() ? nullptr : fixed.data(), target}; }
    sts_speaker_mix view_mix() const { return mix.view(); }
    sts_gain_plan view_gain() const { return sts_gain_plan{gain_db.empty() ? nullptr : gain_db.data(), ramp_ms}; }
    sts_pitch_plan view_pitch() const { return sts_pitch_plan{cents.empty() ? nullptr : cents.data()}; }
};

// was a table that was set for the phoneme counts set_n set for this batch?
inline bool table_matches(const std::vector<int32_t>& set_n, int B, const int32_t* n) {
    if ((int)set_n.size() != B) return false;
    for (int b = 0; b < B; b++)
        if (set_n[(size_t)b] != n[b]) return false;
    return true;
}
// what a call answers when it was not (a speaker mix has no phoneme counts: every_n false)
inline std::string other_batch_message(const char* table, bool every_n = true) {
    return std::string("the ") + table + " was set for another batch (" + (every_n ? "B and every n[b] must match)" : "B must match)");
}

// The staging block of a run (Engine::run_setup): geometry, scales, seeds, ids and the tables, on the device and mirrored in pinned host
// memory, uploaded by the run's one host-to-device copy.  Offsets in 32-bit words from the block's (256-byte aligned) base, in section
// order; a section the run does not have is empty, at the offset of the next.
//   meta 9B + 8 | ls B | ns B | nsw B | seed 2B (uint64: 12B + 8 words in, 8-byte aligned) | ids Ttot | mix mix_words |
//   gain_q Ttot | gain_h B (gain_words == Ttot + B, or 0) | join_sil B | plan_rate Ttot | plan_fixed Ttot | plan_target B | forced Ttot
// `forced` is what the durations kernel reads: uploaded forced durations, or what the plan kernel writes there.  A plan and forced
// durations never come together, so on the pinned side forced durations stand where a plan's arrays otherwise would and the copy ends
// behind whichever is there: copy_words is the block without `forced` unless forced durations are uploaded.
struct StageLayout {
    size_t meta = 0, ls, ns, nsw, seed, ids, mix, gain_q, gain_h, join_sil, plan_rate, plan_fixed, plan_target, forced;
    size_t words, copy_words;
    StageLayout(size_t B, size_t Ttot, size_t mix_words, size_t gain_words, bool join, bool plan, bool have_forced) {
        ls = 9 * B + 8; ns = ls + B; nsw = ns + B; seed = nsw + B; ids = seed + 2 * B;
        mix = ids + Ttot;
        gain_q = mix + mix_words; gain_h = gain_q + (gain_words ? Ttot : 0);
        join_sil = gain_q + gain_words;
        plan_rate = join_sil + (join ? B : 0); plan_fixed = plan_rate + (plan ? Ttot : 0); plan_target = plan_fixed + (plan ? Ttot : 0);
        forced = plan_target + (plan ? B : 0);
        words = forced + Ttot;
        copy_words = have_forced ? words : forced;
    }
};

}  // namespace sts
