// The stream-table rules (h2o_amd/csrc/hhuff_h2streams.h: the code the kernel runs) on the host, as a stand-alone
// program to build with -fsanitize=address,undefined and run directly:
//     h2streams_host CASES MUTATIONS
// CASES: as tests/test_h2streams_host.py writes them from tests/h2streams_corpora.py, one connection a block of lines --
//     C nsteps max_streams max_streams_for_priority active_stream_window_size max_entries max_request_entity_size flags
//     per step:  S iws rep_cap(-1: the bound) nctl(-1: all) nframes nblocks nops nsends
//                F type flags stream_id length ctl.a ctl.b ctl.flags block(-1: none) control-reply-hex
//                B stream_id flags first_frame nframes bstatus exists_map content_length method-hex path-hex host
//                O stream_id op arg          T stream_id sent
//     E status err nstr  nev x (flags status a)  nop x (flags status a)  replies-hex  the four counters
//       nstreams x (id state body output_window input_window bytes_unnotified)          (of the last step)
// ("-": no bytes, "~": no such field.)  Every step is laid out as the calls in front leave it, each array in a heap block
// of exactly its size, and walked against a slab of exactly hhuff_h2_streams_scratch_size; the outcome must be the
// expected one.  Then the table alone: seeded inserts and removals against a std::map, at sizes that fill it.  Then
// MUTATIONS times a seeded case with one hostile change to a frame, control, block or request record, an offset, or
// the reply capacity.  Every walk is checked for what the kernel relies on: events and reply bytes only where they
// belong, canaries behind them untouched, the table's count equal to its entries, every entry found from its home.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "hhuff_h2streams.h"

using namespace hhuff;

static void fail(const char* what, size_t c, long a, long b) {
    printf("FAIL: %s (case %zu: %ld, %ld)\n", what, c, a, b);
    exit(1);
}

struct Ev3 {
    uint32_t flags;
    int32_t status;
    uint32_t a;
};
struct FrameIn {
    uint32_t type, flags, sid, length, a, b, cflags;
    long block;
    std::vector<uint8_t> reply;
};
struct BlockIn {
    uint32_t sid, flags, first, nframes;
    int32_t bstatus;
    uint32_t exists;
    uint64_t cl;
    bool has_method, has_path;
    std::vector<uint8_t> method, path;
    uint32_t host;
};
struct StepIn {
    uint32_t iws;
    long rep_cap, nctl;
    std::vector<FrameIn> frames;
    std::vector<BlockIn> blocks;
    std::vector<hhuff_h2_stream_op_t> ops;
    std::vector<std::pair<uint32_t, uint32_t>> sends;
};
struct StreamOut {
    uint32_t id, state, body;
    int64_t out_w, in_w;
    uint32_t unnotified;
};
struct Case {
    h2s::Cfg P;
    std::vector<StepIn> steps;
    int32_t status;
    uint32_t err, nstr;
    std::vector<Ev3> events, op_events;
    std::vector<uint8_t> replies;
    uint32_t counters[4];
    std::vector<StreamOut> streams;
};

static std::vector<uint8_t> unhex(const char* s, bool* present = nullptr) {
    std::vector<uint8_t> v;
    if (present) *present = strcmp(s, "~") != 0;
    if (strcmp(s, "-") == 0 || strcmp(s, "~") == 0) return v;
    for (; s[0] && s[1]; s += 2) {
        unsigned x;
        sscanf(s, "%2x", &x);
        v.push_back((uint8_t)x);
    }
    return v;
}

constexpr uint8_t kCanary = 0xC7;

template <class T>
struct Block {  // n records in a heap block of exactly that size (one byte for none)
    T* p;
    size_t n;
    explicit Block(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) { memset((void*)p, 0, n_ * sizeof(T)); }
    ~Block() { free(p); }
    Block(const Block&) = delete;
};

// One step's arrays, laid out as the three calls leave them for a call with this one connection.
struct Arrays {
    Block<hhuff_h2_frame_t> frames;
    Block<hhuff_h2_ctl_t> ctl;
    Block<hhuff_h2_block_t> blocks;
    Block<int32_t> bstatus;
    Block<hhuff_request_t> req;
    Block<uint32_t> blk_off, value_off, value_len;
    Block<uint8_t> ctl_rep, arena;
    Block<hhuff_h2_stream_op_t> ops;
    Arrays(const StepIn& s, size_t nfields, size_t nrep, size_t narena)
        : frames(s.frames.size()), ctl(s.frames.size()), blocks(s.frames.size()), bstatus(s.frames.size()), req(s.frames.size()),
          blk_off(s.frames.size() + 1), value_off(nfields), value_len(nfields), ctl_rep(nrep), arena(narena), ops(s.ops.size()) {}
};

struct Outcome {
    h2s::Result R;
    std::vector<hhuff_h2_sev_t> sev, op_sev;
    std::vector<uint8_t> rep;
};

// what a mutation does to the arrays in front of the walk
struct Mutation {
    int kind = -1;
    uint32_t index = 0, field = 0, value = 0;
};

static void check_table(const h2s::Table& T, size_t id) {
    uint32_t n = 0;
    for (uint32_t i = 0; i <= T.mask; ++i) {
        const uint32_t s = T.ent[i].stream_id;
        if (s == 0) continue;
        ++n;
        if (h2s::find(T, s) != i) fail("an entry is not found from its home", id, s, i);
    }
    if (n != T.head->count || n > T.max_entries) fail("the table's count", id, n, T.head->count);
}

static Outcome run_step(const h2s::Cfg& P, const StepIn& s, const h2s::Table& T, bool fresh, const Mutation& mu, size_t id) {
    const uint32_t n = (uint32_t)s.frames.size();
    size_t nrep = 0, narena = 0;
    for (const FrameIn& f : s.frames) nrep += f.reply.size();
    for (const BlockIn& b : s.blocks) narena += b.method.size() + b.path.size();
    const size_t nfields = 2 * s.blocks.size();
    Arrays A(s, nfields, nrep, narena);
    size_t rp = 0, ap = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const FrameIn& f = s.frames[i];
        A.frames.p[i] = hhuff_h2_frame_t{0, f.length, f.sid, (uint8_t)f.type, (uint8_t)f.flags, 0, 0, 0, f.block < 0 ? ~0u : (uint32_t)f.block, 0};
        A.ctl.p[i] = hhuff_h2_ctl_t{f.a, f.b, 0, 0, (uint8_t)f.cflags, (uint8_t)f.reply.size()};
        if (!f.reply.empty()) memcpy(A.ctl_rep.p + rp, f.reply.data(), f.reply.size());
        rp += f.reply.size();
    }
    for (uint32_t b = 0; b < s.blocks.size(); ++b) {
        const BlockIn& k = s.blocks[b];
        A.blocks.p[b] = hhuff_h2_block_t{k.sid, k.sid, k.flags, 0, 16, 0, k.first, k.nframes};
        A.bstatus.p[b] = k.bstatus;
        hhuff_request_t q{};
        q.content_length = k.cl, q.exists_map = k.exists;
        q.method = q.scheme = q.authority = q.path = q.protocol = q.expect = -1;
        A.blk_off.p[b] = 2 * b;
        uint32_t f = 0;
        if (k.has_method) {
            q.method = (int32_t)f;
            A.value_off.p[2 * b + f] = (uint32_t)ap, A.value_len.p[2 * b + f] = (uint32_t)k.method.size();
            if (!k.method.empty()) memcpy(A.arena.p + ap, k.method.data(), k.method.size());
            ap += k.method.size(), ++f;
        }
        if (k.has_path) {
            q.path = (int32_t)f;
            A.value_off.p[2 * b + f] = (uint32_t)ap, A.value_len.p[2 * b + f] = (uint32_t)k.path.size();
            if (!k.path.empty()) memcpy(A.arena.p + ap, k.path.data(), k.path.size());
            ap += k.path.size(), ++f;
        }
        if (k.host || (k.exists & 8u)) q.authority = 0;
        A.req.p[b] = q;
    }
    for (size_t b = s.blocks.size(); b <= n; ++b) A.blk_off.p[b] = (uint32_t)nfields;
    for (size_t k = 0; k < s.ops.size(); ++k) A.ops.p[k] = s.ops[k];
    uint32_t rep_cap = s.rep_cap < 0 ? (uint32_t)hhuff_h2_streams_reply_bound(n, s.ops.size()) : (uint32_t)s.rep_cap;
    uint32_t walked = s.nctl < 0 ? n : ((uint32_t)s.nctl < n ? (uint32_t)s.nctl : n);
    uint32_t b1 = (uint32_t)s.blocks.size();
    // the hostile change: a word of one record, an offset, or a bound -- never one that the kernel's own clamps
    // (hhuff_h2streams.hip) would have caught in front of the walk
    if (mu.kind == 0 && n) ((uint32_t*)&A.frames.p[mu.index % n])[mu.field % 8] = mu.value;
    if (mu.kind == 1 && n) ((uint32_t*)&A.ctl.p[mu.index % n])[mu.field % 4] = mu.value;
    if (mu.kind == 2 && b1) ((uint32_t*)&A.blocks.p[mu.index % b1])[mu.field % 8] = mu.value;
    if (mu.kind == 3 && b1) ((uint32_t*)&A.req.p[mu.index % b1])[mu.field % 12] = mu.value;
    if (mu.kind == 4 && b1) A.bstatus.p[mu.index % b1] = (int32_t)mu.value;
    if (mu.kind == 5) A.blk_off.p[mu.index % (n + 1)] = mu.value;
    if (mu.kind == 6 && nfields) (mu.field & 1 ? A.value_off.p : A.value_len.p)[mu.index % nfields] = mu.value;
    if (mu.kind == 7) rep_cap = mu.value % (rep_cap + 2u);
    if (mu.kind == 8 && !s.ops.empty()) ((uint32_t*)&A.ops.p[mu.index % s.ops.size()])[mu.field % 4] = mu.value;
    if (mu.kind == 9) b1 = mu.value % (n + 1u);  // (the block range, clamped to frm_cap as the kernel clamps it)
    Block<hhuff_h2_sev_t> sev(n), op_sev(s.ops.size());
    memset((void*)sev.p, kCanary, n * sizeof(hhuff_h2_sev_t));
    memset((void*)op_sev.p, kCanary, s.ops.size() * sizeof(hhuff_h2_sev_t));
    Block<uint8_t> rep(rep_cap);
    memset(rep.p, kCanary, rep_cap);
    h2s::Conn C{};
    C.in = nullptr, C.in_size = nfields, C.frames = A.frames.p, C.ctl = A.ctl.p, C.f0 = 0, C.n = walked;
    C.ctl_rep = A.ctl_rep.p, C.ctl_rep_len = (uint32_t)nrep;
    C.blocks = A.blocks.p, C.bstatus = A.bstatus.p, C.req = A.req.p, C.b0 = 0, C.b1 = b1;
    C.arena = A.arena.p, C.arena_size = narena, C.blk_off = A.blk_off.p, C.value_off = A.value_off.p, C.value_len = A.value_len.p;
    C.initial_window_size = s.iws;
    C.ops = A.ops.p, C.nops = (uint32_t)s.ops.size();
    C.sev = sev.p, C.op_sev = op_sev.p, C.rep = rep.p, C.rep_cap = rep_cap;
    Outcome o;
    h2s::walk(C, P, T, fresh, o.R);
    const h2s::Result& R = o.R;
    if (R.nstr > walked || R.rep_len > rep_cap) fail("result range", id, R.nstr, R.rep_len);
    const bool own = R.status == HHUFF_H2ST_SPACE || R.status == HHUFF_H2ST_EINVAL || R.status == HHUFF_H2ST_EFULL;
    const uint32_t written = R.nstr + (R.status != 0 && !own ? 1u : 0u);
    if (R.status == 0 && R.nstr != walked) fail("no failure, yet frames left", id, R.nstr, walked);
    for (size_t k = (size_t)written * sizeof(hhuff_h2_sev_t); k < (size_t)n * sizeof(hhuff_h2_sev_t); ++k)
        if (((const uint8_t*)sev.p)[k] != kCanary) fail("an event behind the stop written", id, (long)k, written);
    for (uint32_t k = R.rep_len; k < rep_cap; ++k)
        if (rep.p[k] != kCanary) fail("reply region written behind rep_len", id, k, R.rep_len);
    check_table(T, id);
    o.sev.assign(sev.p, sev.p + written);
    for (size_t k = 0; k < s.ops.size(); ++k) {
        bool untouched = true;  // (the ops behind a stop for want of room)
        for (size_t q = 0; q < sizeof(hhuff_h2_sev_t); ++q) untouched = untouched && ((const uint8_t*)&op_sev.p[k])[q] == kCanary;
        if (untouched) break;
        o.op_sev.push_back(op_sev.p[k]);
    }
    o.rep.assign(rep.p, rep.p + R.rep_len);
    return o;
}

static void book_sends(const h2s::Table& T, const StepIn& s) {
    if (s.sends.empty()) return;
    const size_t n = s.sends.size();
    Block<hhuff_h2_send_t> sends(n);
    Block<hhuff_h2_sent_t> sent(n);
    Block<uint8_t> miss(n);
    for (size_t r = 0; r < n; ++r) sends.p[r].stream_id = s.sends[r].first, sent.p[r].sent = s.sends[r].second;
    h2s::fill_sends(T, sends.p, (uint32_t)n, miss.p);
    h2s::commit_sent(T, sends.p, sent.p, (uint32_t)n);
}

struct Slab {
    uint8_t* p;
    h2s::Table T;
    explicit Slab(uint32_t max_entries) : p((uint8_t*)malloc(h2s::slab_size(max_entries))), T(h2s::table_at(p, max_entries)) {
        memset(p, kCanary, h2s::slab_size(max_entries));
    }
    ~Slab() { free(p); }
};

static void run_case(const Case& c, size_t id) {
    Slab slab(c.P.max_entries);
    Outcome o;
    for (size_t k = 0; k < c.steps.size(); ++k) {
        if (k != 0) book_sends(slab.T, c.steps[k]);
        o = run_step(c.P, c.steps[k], slab.T, k == 0, Mutation{}, id);
    }
    const h2s::Result& R = o.R;
    if (R.status != c.status || R.err != c.err || R.nstr != c.nstr) fail("status / nstr", id, R.status, R.nstr);
    if (o.sev.size() != c.events.size()) fail("events written", id, (long)o.sev.size(), (long)c.events.size());
    for (size_t i = 0; i < c.events.size(); ++i)
        if (o.sev[i].flags != c.events[i].flags || o.sev[i].status != c.events[i].status || o.sev[i].a != c.events[i].a)
            fail("event", id, (long)i, o.sev[i].flags);
    if (o.op_sev.size() != c.op_events.size()) fail("op events written", id, (long)o.op_sev.size(), (long)c.op_events.size());
    for (size_t i = 0; i < c.op_events.size(); ++i)
        if (o.op_sev[i].flags != c.op_events[i].flags || o.op_sev[i].status != c.op_events[i].status) fail("op event", id, (long)i, o.op_sev[i].status);
    if (o.rep != c.replies) fail("replies", id, (long)o.rep.size(), (long)c.replies.size());
    const h2s::Head& H = *slab.T.head;
    if (H.pull_max_open != c.counters[0] || H.push_max_open != c.counters[1] || H.pull_open != c.counters[2] || H.priority_open != c.counters[3])
        fail("counters", id, H.pull_open, H.priority_open);
    if (H.count != c.streams.size()) fail("streams left", id, H.count, (long)c.streams.size());
    for (const StreamOut& s : c.streams) {
        const uint32_t i = h2s::find(slab.T, s.id);
        if (i == h2s::kNone) fail("stream missing", id, s.id, 0);
        const h2s::Entry& E = slab.T.ent[i];
        if (E.state != s.state || E.body != s.body || E.output_window != s.out_w || E.input_window != s.in_w || E.bytes_unnotified != s.unnotified)
            fail("stream state", id, s.id, (long)E.input_window);
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// the table alone against a std::map: at max_entries streams every one is found, a removal keeps the others reachable
static void table_against_map(uint32_t max_entries, uint32_t rounds) {
    Slab slab(max_entries);
    h2s::clear(slab.T);
    std::map<uint32_t, uint32_t> ref;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t id = 1u + rnd() % (4u * max_entries);
        const uint32_t slot = h2s::find(slab.T, id);
        if ((slot != h2s::kNone) != (ref.count(id) != 0)) fail("table find", max_entries, id, r);
        if (slot != h2s::kNone) {
            if (slab.T.ent[slot].bytes_unnotified != ref[id]) fail("table payload", max_entries, id, r);
            if (rnd() & 1) {
                h2s::remove(slab.T, slot), --slab.T.head->count;
                ref.erase(id);
            }
        } else if (ref.size() < max_entries) {
            h2s::Entry E{};
            E.stream_id = id, E.bytes_unnotified = r;
            h2s::insert(slab.T, E), ++slab.T.head->count;
            ref[id] = r;
        }
        if ((r & 63u) == 0) check_table(slab.T, max_entries);
    }
    check_table(slab.T, max_entries);
    for (const auto& kv : ref)
        if (h2s::find(slab.T, kv.first) == h2s::kNone) fail("table lost an entry", max_entries, kv.first, 0);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const long mutations = atol(argv[2]);
    std::vector<Case> cases;
    static char w[1 << 18], w2[1 << 12];
    char tag;
    while (fscanf(f, " %c", &tag) == 1) {
        if (tag == 'C') {
            Case c{};
            unsigned nsteps, ms, mp, act, me, fl;
            unsigned long long ent;
            if (fscanf(f, "%u %u %u %u %u %llu %u", &nsteps, &ms, &mp, &act, &me, &ent, &fl) != 7) return 2;
            c.P = h2s::Cfg{ms, mp, act - h2s::kHostStreamWindow, fl, me, ent};
            c.steps.resize(nsteps);
            cases.push_back(c);
            size_t k = 0;
            for (; k < nsteps; ++k) {
                StepIn& s = cases.back().steps[k];
                unsigned iws, nf, nb, no, ns;
                if (fscanf(f, " S %u %ld %ld %u %u %u %u", &iws, &s.rep_cap, &s.nctl, &nf, &nb, &no, &ns) != 7) return 2;
                s.iws = iws;
                for (unsigned i = 0; i < nf; ++i) {
                    FrameIn x;
                    if (fscanf(f, " F %u %u %u %u %u %u %u %ld %262143s", &x.type, &x.flags, &x.sid, &x.length, &x.a, &x.b, &x.cflags, &x.block, w) != 9) return 2;
                    x.reply = unhex(w);
                    s.frames.push_back(x);
                }
                for (unsigned i = 0; i < nb; ++i) {
                    BlockIn x;
                    unsigned long long cl;
                    if (fscanf(f, " B %u %u %u %u %d %u %llu %4095s", &x.sid, &x.flags, &x.first, &x.nframes, &x.bstatus, &x.exists, &cl, w2) != 8) return 2;
                    x.cl = cl, x.method = unhex(w2, &x.has_method);
                    if (fscanf(f, " %4095s %u", w2, &x.host) != 2) return 2;
                    x.path = unhex(w2, &x.has_path);
                    s.blocks.push_back(x);
                }
                for (unsigned i = 0; i < no; ++i) {
                    hhuff_h2_stream_op_t op{};
                    if (fscanf(f, " O %u %u %u", &op.stream_id, &op.op, &op.arg) != 3) return 2;
                    s.ops.push_back(op);
                }
                for (unsigned i = 0; i < ns; ++i) {
                    unsigned sid, n;
                    if (fscanf(f, " T %u %u", &sid, &n) != 2) return 2;
                    s.sends.push_back({sid, n});
                }
            }
        } else if (tag == 'E') {
            Case& c = cases.back();
            unsigned nev;
            if (fscanf(f, "%d %u %u %u", &c.status, &c.err, &c.nstr, &nev) != 4) return 2;
            for (unsigned i = 0; i < nev; ++i) {
                Ev3 e;
                if (fscanf(f, "%u %d %u", &e.flags, &e.status, &e.a) != 3) return 2;
                c.events.push_back(e);
            }
            if (fscanf(f, "%u", &nev) != 1) return 2;
            for (unsigned i = 0; i < nev; ++i) {
                Ev3 e;
                if (fscanf(f, "%u %d %u", &e.flags, &e.status, &e.a) != 3) return 2;
                c.op_events.push_back(e);
            }
            unsigned ns;
            if (fscanf(f, " %262143s %u %u %u %u %u", w, &c.counters[0], &c.counters[1], &c.counters[2], &c.counters[3], &ns) != 6) return 2;
            c.replies = unhex(w);
            for (unsigned i = 0; i < ns; ++i) {
                StreamOut s;
                long long ow, iw;
                if (fscanf(f, "%u %u %u %lld %lld %u", &s.id, &s.state, &s.body, &ow, &iw, &s.unnotified) != 6) return 2;
                s.out_w = ow, s.in_w = iw;
                c.streams.push_back(s);
            }
        } else {
            return 2;
        }
    }
    fclose(f);
    for (size_t i = 0; i < cases.size(); ++i) run_case(cases[i], i);
    printf("%zu cases\n", cases.size());
    for (uint32_t me : {1u, 2u, 3u, 7u, 16u, 100u}) table_against_map(me, 20000);
    printf("tables of 1 .. 100 entries against a map\n");
    long refused = 0;
    for (long m = 0; m < mutations && !cases.empty(); ++m) {
        const size_t id = rnd() % cases.size();
        const Case& c = cases[id];
        Slab slab(c.P.max_entries);
        const size_t victim = rnd() % c.steps.size();
        for (size_t k = 0; k < c.steps.size(); ++k) {
            Mutation mu;
            if (k == victim) {
                static const uint32_t edge[] = {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0xfffffffeu, 3u, 9u, 65535u};
                mu.kind = (int)(rnd() % 10u), mu.index = rnd(), mu.field = rnd();
                mu.value = rnd() & 1 ? edge[rnd() % 10u] : rnd() >> (rnd() % 32u);
            }
            if (k != 0) book_sends(slab.T, c.steps[k]);
            const Outcome o = run_step(c.P, c.steps[k], slab.T, k == 0, mu, id);
            if (o.R.status == HHUFF_H2ST_EINVAL) ++refused;
        }
    }
    printf("%ld mutations, %ld refused as out of range\n", mutations, refused);
    printf("ok: h2streams_host\n");
    return 0;
}
