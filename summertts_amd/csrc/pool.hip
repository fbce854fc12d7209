// pool.hip -- request scheduler over several engines on one GPU ("batch scheduler / packed
// varlen layout").  The reference synthesises one utterance per blocking call (SynthesizerTrn.cpp:323); a
// server in front of an MI355X wants (a) the latency-bound text side of one request overlapped with the
// decoder of another and (b) queued requests folded into one packed variable-length batch.  A pool owns
// N engines (one HIP stream set each, weights replicated: ~116 MB per engine out of 288 GB), one worker
// thread per engine, and one FIFO: a free worker takes the oldest request plus up to max_batch - 1 further
// queued ones, runs them as ONE Engine::run batch and completes their tickets.
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "engine.hpp"

using namespace sts;

namespace {
struct Request {
    int64_t ticket = 0;
    std::vector<int32_t> ids; int32_t sid = 0; float ls = 1.f;
    Engine::Noise noise;               // sts_pool_submit_ex: this request's sampling noise
    UttTables tab;                     // sts_pool_submit_plan / _mix / _gain / _pitch / _stream_ex: this request's own tables
    // sts_pool_submit_joined: a paragraph -- its sentences (ids / sid / ls above stay empty), the join (gaps copied: join.gap_frames points
    // into them, or is null) -- run as its own packed batch; sentence b samples with noise.seed + b
    bool joined = false; std::vector<std::vector<int32_t>> sent_ids; std::vector<int32_t> sent_sid; std::vector<float> sent_ls;
    std::vector<int32_t> gaps; sts_join join{nullptr, 0, 0, 0.f};
    // sts_pool_submit_stream: chunks go to cb (on the worker thread); the ticket completes with pcm = null, n = samples delivered
    bool stream = false; int32_t chunk = 0; sts_chunk_cb cb = nullptr; void* user = nullptr;
    // result
    bool done = false, waited = false; int rc = STS_OK; std::string err;
    int16_t* pcm = nullptr; int32_t n = 0;
};
}  // namespace

struct sts_pool {
    std::vector<std::unique_ptr<Engine>> engines;
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<std::shared_ptr<Request>> queue;
    std::map<int64_t, std::shared_ptr<Request>> pending;   // submitted, not yet collected
    int64_t next_ticket = 1;
    int max_batch = 8;
    int loud_mode = 0;                 // sts_pool_set_loudness (streaming requests are refused while it is 2)
    int eq_bands = 0;                  // sts_pool_set_eq (streaming requests are refused while it is not 0)
    bool eq_streaming = false;         // sts_pool_set_eq_streaming (... unless this is on)
    bool stop = false;
    int64_t batches = 0, requests = 0;
    bool stream_admission = false;     // sts_pool_set_stream_admission: streamed groups run as open streams (run_open_group)
    int64_t stream_groups = 0, admitted_midstream = 0;      // sts_pool_stream_stats

    void worker(int k) {
        Engine& eng = *engines[k];
        (void)hipSetDevice(eng.device);
        for (;;) {
            std::vector<std::shared_ptr<Request>> take;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || !queue.empty(); });
                if (stop && queue.empty()) return;
                // a batch is a run of the FIFO's head: whole-utterance requests, or streaming requests of one chunk size -- never both; a
                // joined request is a batch by itself
                const bool st = queue.front()->stream; const int32_t ch = queue.front()->chunk;
                if (queue.front()->joined) { take.push_back(queue.front()); queue.pop_front(); }
                else while (!queue.empty() && (int)take.size() < max_batch && !queue.front()->joined && queue.front()->stream == st && (!st || queue.front()->chunk == ch)) {
                    take.push_back(queue.front()); queue.pop_front();
                }
            }
            if (take.front()->joined) { run_joined_request(eng, *take.front()); cv_done.notify_all(); continue; }
            if (take.front()->stream) {
                // (the settings only change while no request is outstanding.  With bands set a streamed request is here only with
                // eq_streaming on -- submit refuses it otherwise -- and the open stream then runs the EQ from per-slot state)
                if (stream_admission && loud_mode == 0 && (eq_bands == 0 || eq_streaming)) run_open_group(eng, take); else run_stream_group(eng, take);
                cv_done.notify_all();
                continue;
            }
            // run `grp` as one packed batch; on failure of a multi-request batch, re-run its members one by one so
            // that a bad request (e.g. an id outside the vocabulary) only fails itself
            auto run_group = [&](const std::vector<std::shared_ptr<Request>>& grp, auto&& self) -> void {
                const int B = (int)grp.size();
                std::vector<const int32_t*> idp(B); std::vector<int32_t> n(B), sid(B); std::vector<float> ls(B);
                eng.noise_utt.resize(B);
                for (int b = 0; b < B; b++) {
                    idp[b] = grp[b]->ids.data(); n[b] = (int32_t)grp[b]->ids.size(); sid[b] = grp[b]->sid; ls[b] = grp[b]->ls;
                    eng.noise_utt[b] = grp[b]->noise;
                }
                int rc = set_group_tables(eng, grp, n.data());
                if (rc == STS_OK) rc = eng.run(B, idp.data(), n.data(), sid.data(), ls.data());
                eng.noise_utt.clear();
                std::vector<int16_t> all;
                if (rc == STS_OK) {
                    all.resize((size_t)(eng.total_samples > 0 ? eng.total_samples : 1));
                    if (eng.h_pcm) memcpy(all.data(), eng.h_pcm, (size_t)eng.total_samples * 2);   // downloaded inside the run
                    else if (!eng.pcm_hbm() || hipMemcpyAsync(all.data(), eng.pcm_hbm(), (size_t)eng.total_samples * 2, hipMemcpyDeviceToHost, eng.stream) != hipSuccess ||
                             hipStreamSynchronize(eng.stream) != hipSuccess)
                        rc = STS_EDEVICE;
                }
                if (rc != STS_OK && B > 1) {
                    for (auto& r : grp) self(std::vector<std::shared_ptr<Request>>{r}, self);
                    return;
                }
                size_t off = 0;
                std::lock_guard<std::mutex> lk(mu);
                for (int b = 0; b < B; b++) {
                    Request& r = *grp[b];
                    r.rc = rc;
                    if (rc == STS_OK) {
                        r.n = eng.n_samples[b];
                        r.pcm = (int16_t*)malloc((size_t)(r.n > 0 ? r.n : 1) * 2);
                        if (r.pcm) memcpy(r.pcm, all.data() + off, (size_t)r.n * 2); else { r.rc = STS_EDEVICE; r.err = "out of host memory"; }
                        off += (size_t)r.n;
                    } else {
                        r.err = eng.error();
                    }
                    r.done = true;
                }
                batches++; requests += B;
            };
            run_group(take, run_group);
            cv_done.notify_all();
        }
    }

    // The tables of a group's members on `eng`, for its next run (or its next admission into a planned open stream): a kind of table is
    // set when a member carries one, and the members without get an empty entry of it (synthesised as without, bit for bit).  On a
    // failure nothing stays pending for another group.
    int set_group_tables(Engine& eng, const std::vector<std::shared_ptr<Request>>& grp, const int32_t* n) {
        std::vector<const UttTables*> members;
        for (auto& r : grp) members.push_back(&r->tab);
        return apply_utt_tables(eng, (int)grp.size(), n, members.data());
    }

    // a paragraph (Engine::run_joined): its sentences as one packed batch of their own, one PCM
    void run_joined_request(Engine& eng, Request& r) {
        const int B = (int)r.sent_ids.size();
        std::vector<const int32_t*> idp(B); std::vector<int32_t> n(B);
        eng.noise_utt.resize(B);
        for (int b = 0; b < B; b++) {
            idp[b] = r.sent_ids[b].data(); n[b] = (int32_t)r.sent_ids[b].size();
            eng.noise_utt[b] = Engine::Noise{r.noise.ns, r.noise.nsw, r.noise.seed + (uint64_t)b};
        }
        int rc = eng.run_joined(B, idp.data(), n.data(), r.sent_sid.data(), r.sent_ls.data(), &r.join);
        eng.noise_utt.clear();
        int16_t* pcm = nullptr;
        const int64_t total = rc == STS_OK ? eng.total_samples : 0;
        if (rc == STS_OK) {
            pcm = (int16_t*)malloc((size_t)(total > 0 ? total : 1) * 2);
            if (!pcm) rc = STS_EDEVICE;
            else if (eng.h_pcm) memcpy(pcm, eng.h_pcm, (size_t)total * 2);   // downloaded inside the run
            else if (!eng.pcm_hbm() || hipMemcpyAsync(pcm, eng.pcm_hbm(), (size_t)total * 2, hipMemcpyDeviceToHost, eng.stream) != hipSuccess ||
                     hipStreamSynchronize(eng.stream) != hipSuccess)
                rc = STS_EDEVICE;
        }
        std::lock_guard<std::mutex> lk(mu);
        r.rc = rc;
        if (rc == STS_OK) { r.pcm = pcm; r.n = (int32_t)total; }
        else { free(pcm); r.err = eng.error().empty() ? "the joined request failed" : eng.error(); }
        r.done = true;
        batches++; requests++;
    }

    // streaming requests as one batched stream (Engine::run_batch_stream).  A member's ticket completes at its last chunk or its stop; a
    // failure before any chunk of the batch has left re-runs the members one by one, a later one completes the unfinished tickets with it
    void run_stream_group(Engine& eng, const std::vector<std::shared_ptr<Request>>& grp) {
        const int B = (int)grp.size();
        std::vector<const int32_t*> idp(B); std::vector<int32_t> n(B), sid(B); std::vector<float> ls(B);
        eng.noise_utt.resize(B);
        for (int b = 0; b < B; b++) {
            idp[b] = grp[b]->ids.data(); n[b] = (int32_t)grp[b]->ids.size(); sid[b] = grp[b]->sid; ls[b] = grp[b]->ls;
            eng.noise_utt[b] = grp[b]->noise;
        }
        struct Ctx { sts_pool* p; Engine* eng; const std::vector<std::shared_ptr<Request>>* grp; bool any_left; };
        Ctx cx{this, &eng, &grp, false};
        auto cb = [](void* u, int32_t utt, const int16_t* pcm, int32_t ns, int32_t off) -> int {
            Ctx& c = *(Ctx*)u;
            Request& r = *(*c.grp)[utt];
            c.any_left = true;
            r.n += ns;
            const int stop = r.cb(r.user, pcm, ns, off);
            if (stop != 0 || (utt < (int)c.eng->n_samples.size() && r.n >= c.eng->n_samples[utt])) {
                { std::lock_guard<std::mutex> lk(c.p->mu); r.rc = STS_OK; r.done = true; }
                c.p->cv_done.notify_all();
            }
            return stop;
        };
        for (auto& r : grp) r->n = 0;
        int rc = set_group_tables(eng, grp, n.data());        // (sts_pool_submit_stream_ex: the members' own tables)
        if (rc == STS_OK) rc = eng.run_batch_stream(B, idp.data(), n.data(), sid.data(), ls.data(), grp.front()->chunk, cb, &cx, nullptr);
        eng.noise_utt.clear();
        if (rc != STS_OK && B > 1 && !cx.any_left) {
            for (auto& r : grp) run_stream_group(eng, std::vector<std::shared_ptr<Request>>{r});
            return;
        }
        std::lock_guard<std::mutex> lk(mu);
        for (auto& r : grp) {
            if (r->done) continue;
            r->rc = rc;
            if (rc != STS_OK) r->err = eng.error();
            r->done = true;
        }
        batches++; requests += B;
    }

    // sts_pool_set_stream_admission: the group as an OPEN stream on this engine (Engine::stream_open; chunk size of the group, max_live =
    // max_batch, capacity by live_capacity_rule: every slot can hold kLivePoolFrames frames).  The stream is a PLANNED one
    // (sts_stream_open_ex), its phoneme capacity by live_phoneme_rule: every slot can hold a gain plan of kLivePoolPhonemes phonemes --
    // so that planned requests (sts_pool_submit_stream_ex) and plain ones share a group, and a planned one is admitted midstream like
    // any other.  The tables of an admission are set right before it, every time: an admission consumes them whatever its outcome, so
    // the one-by-one retry and a request that came back from the FIFO set theirs again.  Between two steps the worker looks at the
    // FIFO: while its head is a streaming request of the group's chunk size and slots are free it takes up to the free count and admits
    // them.  A head of any other kind stays where it is.  Tickets complete as in run_stream_group: at a member's last chunk or its stop.
    void run_open_group(Engine& eng, const std::vector<std::shared_ptr<Request>>& first) {
        const int32_t chunk = first.front()->chunk;
        if (eng.stream_open(chunk, max_batch, live_capacity_rule(max_batch, kLivePoolFrames), live_phoneme_rule(max_batch, kLivePoolPhonemes)) != STS_OK) { run_stream_group(eng, first); return; }
        struct Ctx { sts_pool* p; std::vector<std::shared_ptr<Request>> slot; std::vector<int32_t> total; };
        Ctx cx{this, std::vector<std::shared_ptr<Request>>((size_t)max_batch), std::vector<int32_t>((size_t)max_batch, 0)};
        auto finish = [this](Request& r, int rc, const std::string& err) {
            { std::lock_guard<std::mutex> lk(mu); r.rc = rc; if (rc != STS_OK) r.err = err; r.done = true; }
            cv_done.notify_all();
        };
        auto cb = [](void* u, int32_t slot, const int16_t* pcm, int32_t ns, int32_t off) -> int {
            Ctx& c = *(Ctx*)u;
            std::shared_ptr<Request> r = c.slot[(size_t)slot];
            r->n += ns;
            const int stop = r->cb(r->user, pcm, ns, off);
            if (stop != 0 || r->n >= c.total[(size_t)slot]) {        // (the engine retires the slot by the same rule: it may be taken again at once)
                c.slot[(size_t)slot].reset();
                { std::lock_guard<std::mutex> lk(c.p->mu); r->rc = STS_OK; r->done = true; }
                c.p->cv_done.notify_all();
            }
            return stop;
        };
        std::vector<std::shared_ptr<Request>> closed;       // members that do not fit the EMPTY pool: as a closed stream behind the drain
        // one admission of `grp` as a packed batch; failing with several members it is retried one by one, so that a bad request fails
        // alone.  No room now: `back` receives the members to return to the head of the FIFO (`closed`: the pool was empty)
        auto admit = [&](const std::vector<std::shared_ptr<Request>>& grp, std::vector<std::shared_ptr<Request>>& back, auto&& self) -> void {
            const int B = (int)grp.size();
            std::vector<const int32_t*> idp((size_t)B); std::vector<int32_t> n((size_t)B), sid((size_t)B), slots((size_t)B, -1), tot((size_t)B, 0);
            std::vector<float> ls((size_t)B); std::vector<sts_stream_noise> nz((size_t)B);
            for (int b = 0; b < B; b++) {
                const Request& r = *grp[(size_t)b];
                idp[(size_t)b] = r.ids.data(); n[(size_t)b] = (int32_t)r.ids.size(); sid[(size_t)b] = r.sid; ls[(size_t)b] = r.ls;
                nz[(size_t)b] = sts_stream_noise{r.noise.ns, r.noise.nsw, r.noise.seed};
            }
            const bool midstream = eng.live_->steps > 0 && eng.live_->live_count() > 0;
            int32_t admitted = 0;
            int rc = set_group_tables(eng, grp, n.data());
            if (rc == STS_OK) rc = eng.stream_admit(B, idp.data(), n.data(), sid.data(), ls.data(), nz.data(), slots.data(), tot.data(), &admitted);
            if (rc != STS_OK || admitted == 0) {
                if (B > 1) { for (auto& r : grp) self(std::vector<std::shared_ptr<Request>>{r}, back, self); return; }
                if (rc != STS_OK) { finish(*grp.front(), rc, eng.error()); std::lock_guard<std::mutex> lk(mu); batches++; requests++; return; }
                if (eng.live_->live_count() == 0) closed.push_back(grp.front()); else back.push_back(grp.front());
                return;
            }
            for (int b = 0; b < B; b++) {
                Request& r = *grp[(size_t)b];
                r.n = 0;
                if (slots[(size_t)b] < 0) { finish(r, STS_OK, ""); continue; }      // (no frames: nothing to deliver)
                cx.slot[(size_t)slots[(size_t)b]] = grp[(size_t)b]; cx.total[(size_t)slots[(size_t)b]] = tot[(size_t)b];
            }
            std::lock_guard<std::mutex> lk(mu);
            batches++; requests += B; if (midstream) admitted_midstream += B;
        };
        { std::lock_guard<std::mutex> lk(mu); stream_groups++; }
        std::vector<std::shared_ptr<Request>> more = first, back;
        bool blocked = false;           // an admission found no room: none is tried again before a slot retires (each costs its front work)
        for (;;) {
            if (!more.empty()) {
                back.clear();
                admit(more, back, admit);
                more.clear();
                if (!back.empty()) {
                    blocked = true;
                    { std::lock_guard<std::mutex> lk(mu); for (auto it = back.rbegin(); it != back.rend(); ++it) queue.push_front(*it); }
                    cv_work.notify_all();            // (back at the head of the FIFO: another worker may be free)
                }
            }
            const int live = eng.live_->live_count();
            if (live > 0) {
                int32_t after = 0;
                const int rc = eng.stream_step(cb, &cx, &after);
                if (rc != STS_OK) {      // the unfinished members end with the error
                    for (auto& r : cx.slot) if (r) { finish(*r, rc, eng.error()); r.reset(); }
                    break;
                }
                if (after < live) blocked = false;
            }
            if (!blocked) {
                std::lock_guard<std::mutex> lk(mu);
                const size_t room = (size_t)eng.live_->free_slots();
                while (!queue.empty() && more.size() < room && queue.front()->stream && !queue.front()->joined && queue.front()->chunk == chunk) {
                    more.push_back(queue.front()); queue.pop_front();
                }
            }
            if (more.empty() && eng.live_->live_count() == 0) break;
        }
        (void)eng.stream_close();
        for (auto& r : closed) run_stream_group(eng, std::vector<std::shared_ptr<Request>>{r});
    }
};

static thread_local std::string g_pool_err;
static int pool_err(int code, const std::string& s) { g_pool_err = s; return code; }

extern "C" {

const char* sts_pool_last_error(void) { return g_pool_err.c_str(); }

int sts_pool_create(const float* blob, int64_t blob_bytes, int device, int n_engines, int max_batch, sts_pool** out) {
    if (!out) return pool_err(STS_EINVAL, "null out pointer");
    *out = nullptr;
    if (n_engines < 1 || n_engines > 16 || max_batch < 1 || max_batch > 1024) return pool_err(STS_EINVAL, "n_engines in 1..16, max_batch in 1..1024");
    sts_pool* p = new (std::nothrow) sts_pool();
    if (!p) return pool_err(STS_EDEVICE, "out of host memory");
    p->max_batch = max_batch;
    for (int k = 0; k < n_engines; k++) {
        p->engines.emplace_back(new Engine());
        p->engines.back()->polite_wait = true;      // worker threads sleep through most of a run's host waits (engine.hpp)
        p->engines.back()->host_pcm = true;
        const int rc = p->engines.back()->init(blob, blob_bytes, device);
        if (rc != STS_OK) { pool_err(rc, p->engines.back()->error()); delete p; return rc; }
    }
    for (int k = 0; k < n_engines; k++) p->workers.emplace_back([p, k] { p->worker(k); });
    *out = p;
    return STS_OK;
}

void sts_pool_destroy(sts_pool* p) {
    if (!p) return;
    { std::lock_guard<std::mutex> lk(p->mu); p->stop = true; }
    p->cv_work.notify_all();
    for (auto& t : p->workers) t.join();
    for (auto& kv : p->pending) if (kv.second->pcm) free(kv.second->pcm);
    delete p;
}

int64_t sts_pool_submit(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale) {
    return sts_pool_submit_ex(p, ids, n, sid, length_scale, 0.f, 0.f, 0);
}

// a request that is not a streaming one into the FIFO: its ticket
static int64_t enqueue(sts_pool* p, const std::shared_ptr<Request>& r) {
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->stop) return pool_err(STS_ESTATE, "pool is shutting down");
        r->ticket = p->next_ticket++;
        p->queue.push_back(r);
        p->pending[r->ticket] = r;
    }
    p->cv_work.notify_one();
    return r->ticket;
}

int64_t sts_pool_submit_ex(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                           float noise_scale_w, uint64_t seed) {
    if (!p || !ids || n <= 0) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    auto r = std::make_shared<Request>();
    r->ids.assign(ids, ids + n); r->sid = sid; r->ls = length_scale; r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    return enqueue(p, r);
}

int64_t sts_pool_submit_plan(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                             float noise_scale_w, uint64_t seed, const float* rate, const int32_t* fixed, int32_t target_frames) {
    if (!p || !ids || n <= 0) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    const char* why = nullptr;
    if (!dur_plan_valid(n, rate, fixed, target_frames, &why)) return pool_err(STS_EINVAL, why);
    auto r = std::make_shared<Request>();
    r->ids.assign(ids, ids + n); r->sid = sid; r->ls = length_scale; r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    r->tab.assign_duration(sts_dur_plan{rate, fixed, target_frames}, n);
    return enqueue(p, r);
}

int64_t sts_pool_submit_mix(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                            float noise_scale_w, uint64_t seed, const sts_speaker_mix* mix) {
    if (!p || !ids || n <= 0) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    const Model& M = p->engines[0]->model;
    const char* why = nullptr;
    if (mix && !speaker_mix_valid(M.is_ms == 1 ? M.spk_num : 0, M.gin, *mix, &why)) return pool_err(STS_EINVAL, why);
    auto r = std::make_shared<Request>();
    r->ids.assign(ids, ids + n); r->sid = sid; r->ls = length_scale; r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    if (mix) r->tab.assign_mix(*mix, M.gin);
    return enqueue(p, r);
}

int64_t sts_pool_submit_gain(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                             float noise_scale_w, uint64_t seed, const sts_gain_plan* plan) {
    if (!p || !ids || n <= 0) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    const char* why = nullptr;
    if (plan && !gain_plan_valid(n, plan->gain_db, plan->ramp_ms, &why)) return pool_err(STS_EINVAL, why);
    auto r = std::make_shared<Request>();
    r->ids.assign(ids, ids + n); r->sid = sid; r->ls = length_scale; r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    if (plan && plan->gain_db) r->tab.assign_gain(*plan, n);      // (a plan without gains is no plan: its ramp is not kept)
    return enqueue(p, r);
}

int64_t sts_pool_submit_joined(sts_pool* p, int32_t B, const int32_t* const* ids, const int32_t* n, const int32_t* sid,
                               const float* length_scale, float noise_scale, float noise_scale_w, uint64_t seed, const sts_join* join) {
    if (!p || !ids || !n || B < 1 || B > (1 << 20)) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    const char* why = nullptr;
    if (!join_valid(B, join, &why)) return pool_err(STS_EINVAL, why);
    for (int b = 0; b < B; b++) if (!ids[b] || n[b] <= 0) return pool_err(STS_EINVAL, "bad request");
    auto r = std::make_shared<Request>();
    r->joined = true;
    r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    r->sent_ids.resize((size_t)B); r->sent_sid.assign((size_t)B, 0); r->sent_ls.assign((size_t)B, 1.f);
    for (int b = 0; b < B; b++) {
        r->sent_ids[b].assign(ids[b], ids[b] + n[b]);
        if (sid) r->sent_sid[b] = sid[b];
        if (length_scale) r->sent_ls[b] = length_scale[b];
    }
    if (join) {
        r->join = *join;
        if (join->gap_frames && B > 1) { r->gaps.assign(join->gap_frames, join->gap_frames + (B - 1)); r->join.gap_frames = r->gaps.data(); }
        else r->join.gap_frames = nullptr;
    }
    return enqueue(p, r);
}

int64_t sts_pool_submit_stream(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                               float noise_scale_w, uint64_t seed, int32_t chunk_frames, sts_chunk_cb cb, void* user) {
    return sts_pool_submit_stream_ex(p, ids, n, sid, length_scale, noise_scale, noise_scale_w, seed, chunk_frames, cb, user, nullptr, nullptr, nullptr);
}

int64_t sts_pool_submit_pitch(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                              float noise_scale_w, uint64_t seed, const sts_pitch_plan* plan) {
    if (!p || !ids || n <= 0) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    const char* why = nullptr;
    if (plan && !pitch_plan_valid(n, plan->cents, &why)) return pool_err(STS_EINVAL, why);
    auto r = std::make_shared<Request>();
    r->ids.assign(ids, ids + n); r->sid = sid; r->ls = length_scale; r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    if (plan) r->tab.assign_pitch(*plan, n);
    return enqueue(p, r);
}

int64_t sts_pool_submit_stream_ex(sts_pool* p, const int32_t* ids, int32_t n, int32_t sid, float length_scale, float noise_scale,
                                  float noise_scale_w, uint64_t seed, int32_t chunk_frames, sts_chunk_cb cb, void* user,
                                  const sts_dur_plan* plan, const sts_speaker_mix* mix, const sts_gain_plan* gain) {
    if (!ids || n <= 0 || chunk_frames <= 0 || !cb) return pool_err(STS_EINVAL, "bad request");
    if (!noise_scale_valid(noise_scale) || !noise_scale_valid(noise_scale_w)) return pool_err(STS_EINVAL, "noise scales must be finite and >= 0");
    const char* why = nullptr;      // (the three checks of sts_pool_submit_plan / _mix / _gain; the two that need no model come first)
    if (plan && !dur_plan_valid(n, plan->rate, plan->fixed, plan->target_frames, &why)) return pool_err(STS_EINVAL, why);
    if (gain && !gain_plan_valid(n, gain->gain_db, gain->ramp_ms, &why)) return pool_err(STS_EINVAL, why);
    if (!p) return pool_err(STS_EINVAL, "bad request");
    const Model& M = p->engines[0]->model;
    if (mix && !speaker_mix_valid(M.is_ms == 1 ? M.spk_num : 0, M.gin, *mix, &why)) return pool_err(STS_EINVAL, why);
    auto r = std::make_shared<Request>();
    r->ids.assign(ids, ids + n); r->sid = sid; r->ls = length_scale; r->noise = Engine::Noise{noise_scale, noise_scale_w, seed};
    r->stream = true; r->chunk = chunk_frames; r->cb = cb; r->user = user;
    if (plan) r->tab.assign_duration(*plan, n);
    if (mix) r->tab.assign_mix(*mix, M.gin);
    if (gain && gain->gain_db) r->tab.assign_gain(*gain, n);      // (as sts_pool_submit_gain)
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->stop) return pool_err(STS_ESTATE, "pool is shutting down");
        if (p->loud_mode != 0) return pool_err(STS_EINVAL, "streaming requests are refused while the pool normalizes loudness (sts_pool_set_loudness mode 0 first)");
        if (p->eq_bands != 0 && !p->eq_streaming)
            return pool_err(STS_EINVAL, "streaming requests are refused while the pool has an equaliser set (sts_pool_set_eq with 0 bands first): an IIR has no finite halo"
                                        " -- or switch the carried-state stream mode on (sts_pool_set_eq_streaming)");
        r->ticket = p->next_ticket++;
        p->queue.push_back(r);
        p->pending[r->ticket] = r;
    }
    p->cv_work.notify_one();
    return r->ticket;
}

int sts_pool_wait(sts_pool* p, int64_t ticket, int16_t** pcm_out, int32_t* n_out) {
    if (!p || !pcm_out || !n_out) return pool_err(STS_EINVAL, "null argument");
    std::shared_ptr<Request> r;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        auto it = p->pending.find(ticket);
        if (it == p->pending.end()) return pool_err(STS_EINVAL, "unknown ticket");
        r = it->second;
        if (r->waited) return pool_err(STS_EINVAL, "ticket is already being waited on");
        r->waited = true;
        p->cv_done.wait(lk, [&] { return r->done; });   // releases the mutex: `it` may be stale afterwards
        p->pending.erase(ticket);
    }
    if (r->rc != STS_OK) { if (r->pcm) free(r->pcm); return pool_err(r->rc, r->err); }
    *pcm_out = r->pcm; *n_out = r->n;
    return STS_OK;
}

int sts_pool_set_output_rate(sts_pool* p, int32_t rate) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    std::lock_guard<std::mutex> lk(p->mu);
    // a request stays pending from submit to wait: with none pending no worker runs, and one batch never mixes rates
    if (!p->pending.empty()) return pool_err(STS_ESTATE, "requests are outstanding: wait for them before changing the output rate");
    ResampleDesign d;
    if (rate != 0 && rate != kNativeRate && !resample_design(kNativeRate, rate, &d)) return pool_err(STS_EINVAL, "output rate must be 0 or an integer in [8000, 48000] with P <= 1024");
    for (auto& e : p->engines) {
        const int rc = e->set_output_rate(rate);
        if (rc != STS_OK) return pool_err(rc, e->error());
    }
    return STS_OK;
}

int sts_pool_set_loudness(sts_pool* p, int mode, float target_lufs, float peak_dbfs) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    if (!loudness_args_valid(mode, target_lufs, peak_dbfs) || mode == 1)
        return pool_err(STS_EINVAL, "pool loudness: mode 0 (off) or 2 (normalize), target in [-70, 0] LUFS, ceiling in [-30, 0] dBFS");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->pending.empty()) return pool_err(STS_ESTATE, "requests are outstanding: wait for them before changing the loudness setting");
    for (auto& e : p->engines) {
        const int rc = e->set_loudness(mode, target_lufs, peak_dbfs);
        if (rc != STS_OK) return pool_err(rc, e->error());
    }
    p->loud_mode = mode;
    return STS_OK;
}

int sts_pool_set_limiter(sts_pool* p, int mode, float gain_db, float ceiling_dbfs, float lookahead_ms) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    if (!limiter_args_valid(mode, gain_db, ceiling_dbfs, lookahead_ms))
        return pool_err(STS_EINVAL, "pool limiter: mode 0 (off) or 1 (on), gain in [-40, 40] dB, ceiling in [-30, 0] dBFS, look-ahead in [0.25, 10] ms");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->pending.empty()) return pool_err(STS_ESTATE, "requests are outstanding: wait for them before changing the limiter setting");
    for (auto& e : p->engines) {
        const int rc = e->set_limiter(mode, gain_db, ceiling_dbfs, lookahead_ms);
        if (rc != STS_OK) return pool_err(rc, e->error());
    }
    return STS_OK;
}

int sts_pool_set_eq(sts_pool* p, int32_t n_bands, const sts_eq_band* bands) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->pending.empty()) return pool_err(STS_ESTATE, "requests are outstanding: wait for them before changing the equaliser");
    const char* why = nullptr;
    for (auto& e : p->engines)          // (all or none: every engine runs at the same rate)
        if (!eq_valid(e->out_rate, n_bands, bands, &why)) return pool_err(STS_EINVAL, why);
    for (auto& e : p->engines) {
        const int rc = e->set_eq(n_bands, bands);
        if (rc != STS_OK) return pool_err(rc, e->error());
    }
    p->eq_bands = n_bands;
    return STS_OK;
}

int sts_pool_set_eq_streaming(sts_pool* p, int enable) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->pending.empty()) return pool_err(STS_ESTATE, "requests are outstanding: wait for them before changing the equaliser's stream mode");
    for (auto& e : p->engines) e->eq_streaming = enable != 0;
    p->eq_streaming = enable != 0;
    return STS_OK;
}

int sts_pool_set_stream_admission(sts_pool* p, int enable) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->pending.empty()) return pool_err(STS_ESTATE, "requests are outstanding: wait for them before changing how streamed groups run");
    p->stream_admission = enable != 0;
    return STS_OK;
}
int sts_pool_get_stream_admission(const sts_pool* p) { return p && p->stream_admission ? 1 : 0; }
int sts_pool_stream_stats(sts_pool* p, int64_t* groups, int64_t* admitted_midstream) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    std::lock_guard<std::mutex> lk(p->mu);
    if (groups) *groups = p->stream_groups;
    if (admitted_midstream) *admitted_midstream = p->admitted_midstream;
    return STS_OK;
}

int sts_pool_stats(sts_pool* p, int64_t* batches, int64_t* requests) {
    if (!p) return pool_err(STS_EINVAL, "null pool");
    std::lock_guard<std::mutex> lk(p->mu);
    if (batches) *batches = p->batches;
    if (requests) *requests = p->requests;
    return STS_OK;
}

}  // extern "C"
