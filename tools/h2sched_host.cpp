// The HTTP/2 scheduler without a GPU: the serial form of h2o_amd/csrc/hhuff_h2sched.h -- the very Sched the kernel
// runs, with the steps over the table (find, first_child, weight_sum, pop, any257, append_unvisited) as plain loops --
// over the fixture's cases with h2o's recorded visits and trees, and over hostile op lists and candidates with the
// tree's invariants checked after every op.  Built with AddressSanitizer and UndefinedBehaviorSanitizer; the table is
// a heap block of exactly max_nodes entries.
//   h2sched_host CASES [ROUNDS]
// CASES, one record a line: "N max_nodes" a new connection; "o id op parent weight exclusive"; "c id bytes window flags";
// "v id bytes" an expected visit; "t id parent weight" an expected stream; "x wc room m active" runs the step and compares.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hhuff_h2sched.h"

using namespace hhuff::h2q;

struct Serial {
    uint32_t uni(uint32_t v) const { return v; }
    void find(const Node* n, uint32_t nhigh, uint32_t id, uint32_t pid, uint32_t& idx, uint32_t& pidx, uint32_t& free_) const {
        idx = pidx = free_ = kNone;
        for (uint32_t i = nhigh; i-- != 0;) {
            if (n[i].id == id) idx = i;
            if (n[i].id == pid && pid != 0) pidx = i;
            if (n[i].id == 0) free_ = i;
        }
    }
    uint32_t first_child(const Node* n, uint32_t nhigh, uint32_t p, uint32_t skip) const {
        uint32_t best = kNone;
        for (uint32_t i = 0; i < nhigh; ++i)
            if (n[i].id != 0 && n[i].parent == p && i != skip && (best == kNone || n[i].aseq < n[best].aseq)) best = i;
        return best;
    }
    uint32_t weight_sum(const Node* n, uint32_t nhigh, uint32_t p) const {
        uint32_t sum = 0;
        for (uint32_t i = 0; i < nhigh; ++i)
            if (n[i].id != 0 && n[i].parent == p) sum += n[i].weight;
        return sum;
    }
    static uint32_t dist(const Node& x, uint32_t qoff) { return x.slot == kSlot257 ? 0u : 1u + ((x.slot - qoff) & (kSlots - 1u)); }
    Popped pop(const Node* n, uint32_t nhigh, uint32_t p, uint32_t qoff) const {
        uint32_t best = kNone, same = 0;
        for (uint32_t i = 0; i < nhigh; ++i) {
            if (n[i].id == 0 || n[i].parent != p || n[i].slot == kUnqueued) continue;
            const uint32_t d = dist(n[i], qoff), bd = best == kNone ? 0 : dist(n[best], qoff);
            if (best == kNone || d < bd || (d == bd && n[i].qseq < n[best].qseq)) best = i;
        }
        if (best == kNone) return Popped{kNone, 0, false};
        for (uint32_t i = 0; i < nhigh; ++i)
            same += n[i].id != 0 && n[i].parent == p && n[i].slot == n[best].slot;
        return Popped{best, dist(n[best], qoff), same > 1};
    }
    bool any257(const Node* n, uint32_t nhigh, uint32_t p) const {
        for (uint32_t i = 0; i < nhigh; ++i)
            if (n[i].id != 0 && n[i].parent == p && n[i].slot == kSlot257) return true;
        return false;
    }
    void append_unvisited(Visits& V) const {
        for (uint32_t j = V.lo; j < V.hi; ++j) {
            if (V.pos[j] != kNone) continue;
            hhuff_h2_send_t S = V.sends[j];
            S.window = 0;
            V.ordered[V.lo + V.n] = S, V.order[V.lo + V.n] = j, V.pos[j] = V.n, ++V.n;
        }
    }
};

static int failures = 0;
#define CHECK(c, ...)                                      \
    do {                                                   \
        if (!(c)) {                                        \
            if (++failures < 20) printf(__VA_ARGS__), printf("   [%s]\n", #c); \
        }                                                  \
    } while (0)

struct Conn {
    Serial w;
    uint32_t max_nodes;
    Node* n;
    uint32_t* cand;
    Sched<Serial> S;
    explicit Conn(uint32_t mn)
        : max_nodes(mn), n((Node*)calloc(mn, sizeof(Node))), cand((uint32_t*)calloc(mn, 4)), S{w, n, cand, fresh_header(mn), mn} {}
    ~Conn() { free(n), free(cand); }
    Conn(const Conn&) = delete;
    uint32_t index_of(uint32_t id) const {
        for (uint32_t i = 0; i < S.h.nhigh; ++i)
            if (n[i].id == id) return i;
        return kNone;
    }
    // what scheduler.c's asserts and lists imply
    void invariants(const char* what) const {
        uint32_t count = 0;
        for (uint32_t i = 0; i < S.h.nhigh; ++i) {
            const Node& x = n[i];
            if (x.id == 0) continue;
            ++count;
            CHECK(node_ok(x, S.h.nhigh), "%s: node %u out of range", what, i);
            uint32_t act = x.self_active, steps = 0;
            for (uint32_t k = 0; k < S.h.nhigh; ++k) act += n[k].id != 0 && n[k].parent == i && n[k].active_cnt != 0;
            CHECK(act == x.active_cnt, "%s: stream %u counts %u, has %u", what, x.id, x.active_cnt, act);
            CHECK((x.active_cnt != 0) == (x.slot != kUnqueued), "%s: stream %u queued %u with count %u", what, x.id, x.slot, x.active_cnt);
            CHECK(x.parent == kRoot || n[x.parent].id != 0, "%s: stream %u under a free entry", what, x.id);
            for (uint32_t t = i; t != kRoot && steps <= max_nodes; t = n[t].parent) ++steps;
            CHECK(steps <= max_nodes, "%s: stream %u in a cycle", what, x.id);
        }
        CHECK(count == S.h.count && (S.h.nhigh == 0 || n[S.h.nhigh - 1].id != 0), "%s: count %u of %u, high %u", what, S.h.count, count, S.h.nhigh);
    }
};

struct Step {
    std::vector<hhuff_h2_sched_op_t> ops;
    std::vector<hhuff_h2_send_t> cands;
    std::vector<long long> visits, tree;
};

static uint32_t run_step(Conn& C, const Step& st, long long wc, long long room, long long m, std::vector<hhuff_h2_send_t>& ordered,
                         std::vector<uint32_t>& order, std::vector<uint32_t>& pos) {
    const uint32_t nc = (uint32_t)st.cands.size();
    ordered.assign(nc, hhuff_h2_send_t{}), order.assign(nc, kNone), pos.assign(nc, kNone);
    memset(C.cand, 0, 4 * (size_t)C.max_nodes);
    Visits V{st.cands.data(), 0, nc, ordered.data(), order.data(), pos.data(), 0};
    return C.S.run(V, m, room, wc);
}

static void fixture(const char* path, unsigned* ncase, unsigned* nstep) {
    FILE* f = fopen(path, "r");
    if (!f) exit(2);
    char line[256];
    Conn* C = nullptr;
    Step st;
    std::vector<hhuff_h2_send_t> ordered;
    std::vector<uint32_t> order, pos;
    while (fgets(line, sizeof line, f)) {
        long long a[6] = {0, 0, 0, 0, 0, 0};
        sscanf(line + 1, "%lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4);
        if (line[0] == 'N') delete C, C = new Conn((uint32_t)a[0]), ++*ncase;
        else if (line[0] == 'o') st.ops.push_back(hhuff_h2_sched_op_t{(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint16_t)a[3], (uint8_t)a[4], 0});
        else if (line[0] == 'c') st.cands.push_back(hhuff_h2_send_t{0, (uint32_t)a[1], (uint32_t)a[0], (int32_t)a[2], (uint32_t)a[3], 0});
        else if (line[0] == 'v') st.visits.push_back(a[0]), st.visits.push_back(a[1]);
        else if (line[0] == 't') st.tree.push_back(a[0]), st.tree.push_back(a[1]), st.tree.push_back(a[2]);
        else if (line[0] == 'x') {
            for (const auto& o : st.ops) CHECK(C->S.apply(o) == 0, "step %u: op %u of stream %u refused", *nstep, o.op, o.stream_id);
            C->invariants("fixture ops");
            const uint32_t nv = run_step(*C, st, a[0], a[1], a[2], ordered, order, pos);
            C->invariants("fixture run");
            CHECK(nv == st.visits.size() / 2, "step %u: %u visits, h2o %zu", *nstep, nv, st.visits.size() / 2);
            long long R = a[1], Wc = a[0];
            for (uint32_t k = 0; k < nv && k < st.visits.size() / 2; ++k) {
                const hhuff_h2_send_t& S = ordered[k];
                const auto F = hhuff::h2d::record(a[2], R, Wc, S.window, S.body_len, S.flags & 1, S.flags & 2, 0);
                CHECK(S.stream_id == st.visits[2 * k] && F.bytes(a[2]) == st.visits[2 * k + 1], "step %u visit %u: stream %u sends %lld, h2o %lld %lld",
                      *nstep, k, S.stream_id, (long long)F.bytes(a[2]), st.visits[2 * k], st.visits[2 * k + 1]);
                R -= F.bytes(a[2]) + 9 * F.count(), Wc -= F.bytes(a[2]);
            }
            CHECK(C->S.is_active() == (a[3] != 0), "step %u: active %d, h2o %lld", *nstep, (int)C->S.is_active(), a[3]);
            CHECK(C->S.h.count == st.tree.size() / 3, "step %u: %u streams, h2o %zu", *nstep, C->S.h.count, st.tree.size() / 3);
            for (size_t k = 0; k + 2 < st.tree.size(); k += 3) {
                const uint32_t i = C->index_of((uint32_t)st.tree[k]);
                if (i == kNone) {
                    CHECK(false, "step %u: stream %lld is missing", *nstep, st.tree[k]);
                    continue;
                }
                const uint32_t pid = C->n[i].parent == kRoot ? 0 : C->n[C->n[i].parent].id;
                CHECK(pid == st.tree[k + 1] && C->n[i].weight == st.tree[k + 2], "step %u: stream %lld under %u weight %u, h2o %lld %lld", *nstep,
                      st.tree[k], pid, C->n[i].weight, st.tree[k + 1], st.tree[k + 2]);
            }
            st = Step(), ++*nstep;
        }
    }
    delete C;
    fclose(f);
}

static uint32_t rng_state = 12345;
static uint32_t rnd(uint32_t n) { return ((rng_state = rng_state * 1664525u + 1013904223u) >> 8) % n; }

// random and malformed ops on small tables: a refused op changes nothing, the invariants hold, nothing leaves the table
static unsigned hostile(unsigned rounds) {
    unsigned nops = 0;
    for (unsigned r = 0; r < rounds; ++r) {
        const uint32_t mn = 1 + rnd(r % 3 == 0 ? 6 : 70);
        Conn C(mn);
        std::vector<Node> before(mn);
        for (unsigned k = 0; k < 400; ++k, ++nops) {
            hhuff_h2_sched_op_t o{1 + rnd(24), 1 + rnd(5), rnd(26), (uint16_t)(1 + rnd(257)), (uint8_t)rnd(2), 0};
            if (o.op > HHUFF_H2Q_REBIND) o.parent_id = 0, o.weight = 0, o.exclusive = 0;
            const uint32_t twist = rnd(40);
            if (twist == 0) o.op = rnd(9);
            if (twist == 1) o.stream_id = rnd(2) ? 0 : 0x80000000u;
            if (twist == 2) o.weight = rnd(2) ? 0 : 258 + rnd(60000);
            if (twist == 3) o.rsv = 1, o.exclusive = (uint8_t)rnd(4);
            if (twist == 4) o.parent_id = rnd(2) ? o.stream_id : 0xFFFFFFFFu;
            memcpy(before.data(), C.n, sizeof(Node) * mn);
            const Header hb = C.S.h;
            const int32_t st = C.S.apply(o);
            if (st != 0)
                CHECK(memcmp(before.data(), C.n, sizeof(Node) * mn) == 0 && memcmp(&hb, &C.S.h, sizeof hb) == 0, "op %u status %d changed the tree", o.op, st);
            CHECK(st == 0 || (st <= HHUFF_H2SC_EINVAL && st >= HHUFF_H2SC_EFULL), "op %u status %d", o.op, st);
            CHECK(st != 0 || op_check(o) == 0, "a malformed op %u passed", o.op);
            C.invariants("hostile op");
            if (k % 16 == 15) {  // candidates: unknown streams, duplicates, id 0, odd flags and windows
                Step s;
                for (uint32_t j = 0, nc = rnd(12); j < nc; ++j)
                    s.cands.push_back(hhuff_h2_send_t{rnd(100), rnd(3) ? rnd(40000) : 0, rnd(28), (int32_t)rnd(50) - 5, rnd(5), rnd(3)});
                std::vector<hhuff_h2_send_t> ordered;
                std::vector<uint32_t> order, pos;
                const uint32_t nv = run_step(C, s, (long long)rnd(60000) - 10, rnd(4) ? rnd(70000) : rnd(12), 16384, ordered, order, pos);
                C.invariants("hostile run");
                CHECK(nv <= s.cands.size(), "more visits than candidates");
                for (uint32_t k2 = 0; k2 < nv; ++k2) CHECK(candidate_ok(ordered[k2].stream_id, ordered[k2].flags), "a visit of a record the framer refuses");
                for (uint32_t j = 0; j < s.cands.size(); ++j)
                    CHECK(pos[j] < s.cands.size() && order[pos[j]] == j && ordered[pos[j]].stream_id == s.cands[j].stream_id, "record %u lost", j);
                for (uint32_t k2 = 0; k2 < nv; ++k2)
                    for (uint32_t k3 = 0; k3 < k2; ++k3) CHECK(ordered[k2].stream_id != ordered[k3].stream_id, "a stream visited twice");
            }
        }
    }
    return nops;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    // the offset table's ends and close's clamp
    CHECK(offset_of(1) == 63u * 65536u && offset_of(256) == 16128u && offset_of(257) == 0 && offset_of(5) == 825754u, "offsets");
    for (uint32_t w = 1; w < 256; ++w) CHECK(offset_of(w) > offset_of(w + 1), "offset %u", w);
    CHECK(handed_weight(257, 257, 257) == 256 && handed_weight(1, 257, 1) == 1 && handed_weight(16, 48, 16) == 5, "handed weights");
    unsigned ncase = 0, nstep = 0;
    fixture(argv[1], &ncase, &nstep);
    const unsigned nops = hostile(argc > 2 ? (unsigned)atoi(argv[2]) : 8);
    if (failures) {
        printf("FAILED: %d checks\n", failures);
        return 1;
    }
    printf("ok: h2sched_host, %u cases, %u steps, %u hostile ops\n", ncase, nstep, nops);
    return 0;
}
