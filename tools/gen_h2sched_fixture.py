#!/usr/bin/env python3
"""Write tests/golden/h2sched.npz: what h2o's own lib/http2/scheduler.c does with scripted tree operations and runs.

    python tools/gen_h2sched_fixture.py REF        REF: the h2o tree (default $H2O_REF)

lib/http2/scheduler.c (and lib/common/memory.c, -ffunction-sections -Wl,--gc-sections) link against the small dump program
below, which is compiled in a temporary directory and removed with it; only the .npz is written.  The program applies the
ops with h2o_http2_scheduler_*, finds a parent as set_priority does (an id that is not open: the root, weight 16, not
exclusive) and runs h2o_http2_scheduler_run when the buffer window is above 0, with a callback that sends frame by frame
as h2o_http2_stream_send_pending_data does and answers as emit_writereq_of_openref does.  Data only; a case is a
connection, a step is one call:
  names               the cases' names, '\\n' between them
  case_first          u32 [ncase + 1]: case k is the steps case_first[k] .. case_first[k + 1]
  op_first, ops       u32 [nstep + 1], u32 [nop, 5]: stream_id, op (include/hhuff.h HHUFF_H2Q_*), parent_id, weight, exclusive
  cand_first, cands   u32 [nstep + 1], i64 [ncand, 4]: stream_id, bytes pending, the stream's window, HHUFF_H2S_* flags
  conn                i64 [nstep, 3]: the connection's window, the room in its buffer, max_frame_size
  visit_first, visits u32 [nstep + 1], i64 [nvisit, 2]: the stream visited and the bytes the visit sent, in h2o's order
  active              u8 [nstep]: h2o_http2_scheduler_is_active(root) after the step
  tree_first, tree    u32 [nstep + 1], u32 [ntree, 3]: after the step every open stream's id, parent id and weight, by id
The cases: the scenarios of t/00unit/lib/http2/scheduler.c (with a visit per step where its callback counts visits),
tree edits, long queues, runs that bail out, and trees around the wave's width."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "h2sched.npz")
OPEN, REBIND, CLOSE, ACTIVATE, DEACTIVATE = 1, 2, 3, 4, 5
M = 16384

DUMP_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h2o/memory.h"
#include "h2o/http2_scheduler.h"

#define MAXID 8192
static struct stream {
    h2o_http2_scheduler_openref_t ref;
    int open, has, flags, id;
    long long bytes, window;
} streams[MAXID];
static h2o_http2_scheduler_node_t root;
static long long Wc, R, M;

static long long buffer_window(void)
{
    if (R < 9)
        return 0;
    return R - 9 < Wc ? R - 9 : Wc;
}

/* h2o_http2_stream_send_pending_data, frame by frame, then emit_writereq_of_openref's answer */
static int cb(h2o_http2_scheduler_openref_t *ref, int *still_is_active, void *arg)
{
    struct stream *s = (void *)ref;
    long long sent = 0, n;
    int final = s->flags & 1, trailers = s->flags & 2, done = 0;
    *still_is_active = 0;
    if (!s->has)
        return buffer_window() > 0 ? 0 : -1;
    while (!done) {
        if (s->window <= 0 || R < 9 || R - 9 <= 0 || Wc <= 0)
            break;
        n = M;
        if (R - 9 < n) n = R - 9;
        if (Wc < n) n = Wc;
        if (s->window < n) n = s->window;
        if (s->bytes < n) n = s->bytes;
        if (n != 0 || (final && !trailers))
            R -= n + 9;
        Wc -= n, s->window -= n, s->bytes -= n, sent += n;
        done = s->bytes == 0;
    }
    printf(" %d:%lld", s->id, sent);
    s->has = 0;
    if (!done && s->window > 0)
        *still_is_active = 1;
    return buffer_window() > 0 ? 0 : -1;
}

int main(void)
{
    char line[256];
    int id, pid, w, e, i;
    while (fgets(line, sizeof(line), stdin) != NULL) {
        struct stream *s;
        h2o_http2_scheduler_node_t *parent;
        switch (line[0]) {
        case 'N':
            memset(streams, 0, sizeof(streams));
            h2o_http2_scheduler_init(&root);
            break;
        case 'O':
        case 'B':
            sscanf(line + 2, "%d %d %d %d", &id, &pid, &w, &e);
            s = streams + id;
            if (pid == 0) {
                parent = &root;
            } else if (streams[pid].open) {
                parent = &streams[pid].ref.node;
            } else {
                parent = &root, w = 16, e = 0;
            }
            if (line[0] == 'O') {
                s->open = 1, s->id = id;
                h2o_http2_scheduler_open(&s->ref, parent, w, e);
            } else {
                h2o_http2_scheduler_rebind(&s->ref, parent, w, e);
            }
            break;
        case 'C':
            sscanf(line + 2, "%d", &id);
            h2o_http2_scheduler_close(&streams[id].ref);
            streams[id].open = 0;
            break;
        case 'A':
            sscanf(line + 2, "%d", &id);
            h2o_http2_scheduler_activate(&streams[id].ref);
            break;
        case 'D':
            sscanf(line + 2, "%d", &id);
            h2o_http2_scheduler_deactivate(&streams[id].ref);
            break;
        case 'S':
            sscanf(line + 2, "%d", &id);
            s = streams + id;
            sscanf(line + 2, "%d %lld %lld %d", &id, &s->bytes, &s->window, &s->flags);
            s->has = 1;
            break;
        case 'X':
            sscanf(line + 2, "%lld %lld %lld", &Wc, &R, &M);
            printf("V");
            if (buffer_window() > 0)
                h2o_http2_scheduler_run(&root, cb, NULL);
            printf(" | %d\nT", h2o_http2_scheduler_is_active(&root));
            for (i = 0; i != MAXID; ++i) {
                streams[i].has = 0;
                if (streams[i].open) {
                    h2o_http2_scheduler_node_t *p = streams[i].ref.node._parent;
                    printf(" %d:%d:%d", i, p == &root ? 0 : ((struct stream *)p)->id, (int)streams[i].ref.weight);
                }
            }
            printf("\n");
            break;
        }
    }
    return 0;
}
"""

BIG = 1 << 20


def step(ops=(), cands=(), wc=BIG, room=BIG, m=M):
    return (list(ops), list(cands), (wc, room, m))


def op(kind, sid, pid=0, w=0, e=0):
    return (sid, kind, pid, w, e)


def opens(specs, activate=True):
    """[(id, parent, weight)] -> OPEN ops, each followed by ACTIVATE"""
    out = []
    for sid, pid, w in specs:
        out.append(op(OPEN, sid, pid, w))
        if activate:
            out.append(op(ACTIVATE, sid))
    return out


def serve(ids, k, first_ops=()):
    """k steps of one visit each: every stream has plenty to send and the connection's window ends with the visit"""
    return [step(first_ops if s == 0 else (), [(i, BIG, BIG, 0) for i in ids], wc=10) for s in range(k)]


def drain(ids, ops=()):
    """one step that visits every active stream once: each has 5 bytes and is done"""
    return step(ops, [(i, 5, BIG, 1) for i in ids])


def cases():
    C = {}
    # t/00unit/lib/http2/scheduler.c
    for name, ws in (("unit_queue", (256, 128, 64)), ("unit_round_robin", (1, 1, 1)), ("unit_priority", (32, 32, 12))):
        ids = [1, 3, 5]
        C[name] = serve(ids, 30, opens([(i, 0, w) for i, w in zip(ids, ws)]))
    C["unit_dependency"] = (serve([1, 3, 5, 7], 12, opens([(1, 0, 32), (3, 0, 32), (5, 1, 12), (7, 1, 6)])) +
                            [drain([1])] + serve([3, 5, 7], 12) + [drain([3, 5])] + serve([7], 3))
    C["unit_exclusive"] = (serve([1, 3, 5], 6, opens([(1, 0, 32), (3, 0, 32)]) + [op(OPEN, 5, 0, 12, 1), op(ACTIVATE, 5)]) +
                           [drain([5])] + serve([1, 3], 6))
    fire = opens([(3, 0, 201), (5, 0, 101), (7, 0, 1), (9, 7, 1), (11, 3, 1)], activate=False)
    C["unit_firefox"] = (serve([13], 5, fire + opens([(13, 11, 22)])) + serve([13, 15, 17], 5, opens([(15, 3, 22), (17, 3, 22)])) +
                         [step((), [(15, 5, BIG, 1), (17, 5, BIG, 1), (13, BIG, BIG, 0)], wc=15)] + serve([13], 3) +
                         serve([13], 3, [op(CLOSE, 15), op(CLOSE, 17)]) + [step([op(CLOSE, 13), op(CLOSE, 3), op(CLOSE, 7)])])
    abc = opens([(1, 0, 6), (3, 1, 5), (5, 1, 4), (7, 5, 3), (9, 5, 2), (11, 7, 1)])
    for e in (0, 1):
        C["unit_reprioritize_%d" % e] = [step(abc)] + serve([1, 3, 5, 7, 9, 11], 8, [op(REBIND, 1, 7, 1, e)]) + [step([op(CLOSE, 1)])]
    C["rebind_grandchild"] = [step(abc)] + serve([1, 3, 5, 7, 9, 11], 8, [op(REBIND, 1, 11, 9, 1)])
    for e in (0, 1):  # onto one's own child: 1 under 5, then 5 under 1, by then its child
        C["rebind_child_%d" % e] = ([step(abc)] + serve([1, 3, 5, 7, 9, 11], 8, [op(REBIND, 1, 5, 2, e)]) +
                                    serve([1, 3, 5, 7, 9, 11], 8, [op(REBIND, 5, 1, 200, e)]))
    C["unit_change_weight"] = (serve([1, 3, 5], 20, opens([(1, 0, 16), (3, 0, 16), (5, 0, 16)])) + serve([1, 3, 5], 20, [op(REBIND, 1, 0, 4)]) +
                               [step((), [(3, 5, BIG, 1), (5, 5, BIG, 1), (1, BIG, BIG, 0)], wc=15)] + serve([1], 4))
    C["unit_exclusive_at_pos"] = serve([1, 3, 5], 9, opens([(1, 0, 16), (3, 0, 16), (5, 0, 16)]) + [op(REBIND, 3, 0, 1, 1)])
    # tree edits
    kids = [(3, 1, 1), (5, 1, 16), (7, 1, 256)]
    for k in (0, 1, 3):
        C["excl_open_%d" % k] = serve([1, 3, 5, 7, 9][:k + 1] + [9], 8, opens([(1, 0, 16)], False) + opens(kids[:k]) + [op(OPEN, 9, 1, 32, 1), op(ACTIVATE, 9)])
    for pw in (1, 16, 257):
        for ws in ((1, 256), (16, 16, 16), (256, 256), (257,)):
            ids = [3 + 2 * i for i in range(len(ws))]
            C["close_%d_%s" % (pw, "_".join(map(str, ws)))] = (
                [step(opens([(1, 0, pw), (21, 0, 16)]) + opens([(i, 1, w) for i, w in zip(ids, ws)]))] + serve([21] + ids, 10, [op(CLOSE, 1)]))
    C["rebind_no_change"] = serve([1, 3], 6, opens([(1, 0, 16), (3, 0, 16)]) + [op(REBIND, 1, 0, 16)])
    C["parent_missing"] = serve([1, 3, 5], 9, opens([(1, 0, 32), (3, 99, 200)]) + [op(OPEN, 5, 1, 7, 1), op(ACTIVATE, 5), op(REBIND, 5, 77, 3, 1)])
    C["w257"] = serve([1, 3, 5, 7, 9], 24, opens([(1, 0, 1), (3, 0, 16), (5, 0, 257), (7, 0, 256), (9, 3, 257)]))
    # queues: deficits and the ring wrap
    for name, ws in (("queue_1_16", (1, 16)), ("queue_1_16_256", (1, 16, 256)), ("queue_16_256_256", (16, 256, 256))):
        ids = [1 + 2 * i for i in range(len(ws))]
        C[name] = serve(ids, 210, opens([(i, 0, w) for i, w in zip(ids, ws)]))
        # a small stream window ends each visit; the next step credits it and activates again
        C[name + "_credit"] = [step(opens([(i, 0, w) for i, w in zip(ids, ws)]) if s == 0 else [op(ACTIVATE, i) for i in ids[::-1]],
                                    [(i, BIG, 7, 0) for i in ids]) for s in range(105)]
    C["inactive_parent"] = serve([3, 5, 7], 24, opens([(1, 0, 8), (9, 0, 8)], False) + opens([(3, 1, 4), (5, 1, 40), (7, 9, 16)]))
    C["deactivate_queued"] = serve([1, 3, 5], 6, opens([(1, 0, 16), (3, 0, 16), (5, 0, 16)]) + [op(DEACTIVATE, 3)]) + serve([1, 3, 5], 6, [op(ACTIVATE, 3), op(DEACTIVATE, 1)])
    # runs
    three = opens([(1, 0, 16), (3, 0, 16), (5, 0, 16)])
    c10 = [(i, 10, BIG, 1) for i in (5, 1, 3)]
    C["bail_conn_window"] = [step(three, c10, wc=20), step((), c10[:1] + c10[2:], wc=100)]
    C["bail_room"] = [step(three, c10, room=9 + 10 + 9 + 10 + 5), step((), c10[:1] + c10[2:], room=8), step((), c10[:1] + c10[2:], room=50)]
    C["entry_window_0"] = [step(three, c10, wc=0), step((), c10, wc=-5), step((), c10, room=9), step((), c10)]
    C["partial_frames"] = [step(three, [(1, 40000, 20000, 1), (3, 0, 5, 1), (5, 7, 0, 1)], room=60000), step([op(ACTIVATE, 5)], [(1, 20000, 30000, 3), (5, 7, 1, 1)])]
    # trees around the wave's width: flat, then a chain under the last stream
    for nn in (1, 63, 64, 65, 130, 300):
        ids = list(range(1, 2 * nn, 2))
        flat = opens([(i, 0, 1 + (i * 7) % 256) for i in ids])
        C["flat_%d" % nn] = [step(flat, [(i, 5 + i % 3, BIG, 1) for i in ids[::-1]]),
                             step([op(ACTIVATE, i) for i in ids] + [op(OPEN, 2 * nn + 2, ids[nn // 2], 9, 1)] if nn != 130 else [op(ACTIVATE, i) for i in ids],
                                  [(i, 5, BIG, 1) for i in ids]), step([op(CLOSE, ids[0])])]
    C["chain_16"] = [step([x for i in range(16) for x in (op(OPEN, 2 * i + 1, 2 * i - 1 if i else 0, 16 + i, 1), op(ACTIVATE, 2 * i + 1))],
                          [(2 * i + 1, 5, BIG, 1) for i in range(16)]),
                     step([op(CLOSE, 5), op(REBIND, 31, 0, 256, 1), op(ACTIVATE, 7), op(ACTIVATE, 31)], [(7, 5, BIG, 1), (31, 5, BIG, 1)])]
    return C


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("H2O_REF", "")
    srcs = [os.path.join(ref, "lib", *p) for p in (("http2", "scheduler.c"), ("common", "memory.c"))]
    if not all(os.path.exists(s) for s in srcs):
        sys.exit("no h2o tree at %r (lib/http2/scheduler.c)" % ref)
    inc = [os.path.join(ref, "include")] + [os.path.join(ref, "deps", d) for d in (
        "picotls/include", "quicly/include", "klib", "golombset", "cloexec", "yoml", "libgkc", "libyrmcds", "picohttpparser",
        "hiredis", "brotli/c/include")]
    C = cases()
    letter = {OPEN: "O", REBIND: "B", CLOSE: "C", ACTIVATE: "A", DEACTIVATE: "D"}
    feed, steps = [], []
    for name, st in C.items():
        feed.append("N")
        for ops, cands, conn in st:
            for sid, kind, pid, w, e in ops:
                feed.append("%s %d %d %d %d" % (letter[kind], sid, pid, w, e) if kind <= REBIND else "%s %d" % (letter[kind], sid))
            feed += ["S %d %d %d %d" % c for c in cands] + ["X %d %d %d" % conn]
            steps.append((ops, cands, conn))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dump_h2sched.c"), os.path.join(tmp, "dump_h2sched")
        with open(src, "w") as f:
            f.write(DUMP_C)
        subprocess.run(["gcc", "-O1", "-w", "-DH2O_USE_LIBUV=0", "-ffunction-sections", "-fdata-sections"] + ["-I" + d for d in inc] +
                       [src] + srcs + ["-Wl,--gc-sections", "-lpthread", "-o", exe], check=True)
        lines = [r for r in subprocess.run([exe], input="\n".join(feed) + "\n", check=True, capture_output=True, text=True).stdout.split("\n") if r]
    assert len(lines) == 2 * len(steps), (len(lines), len(steps))
    visits, active, tree = [], [], []
    for k in range(len(steps)):
        v, t = lines[2 * k].split(), lines[2 * k + 1].split()
        assert v[0] == "V" and v[-2] == "|" and t[0] == "T"
        visits.append([tuple(map(int, x.split(":"))) for x in v[1:-2]])
        active.append(int(v[-1]))
        tree.append([tuple(map(int, x.split(":"))) for x in t[1:]])
    first = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)  # noqa: E731
    flat = lambda rows, w, dt: np.array([x for r in rows for x in r], dt).reshape(-1, w)  # noqa: E731
    np.savez_compressed(
        OUT, names=np.frombuffer("\n".join(C).encode(), np.uint8), case_first=first(list(C.values())),
        op_first=first([s[0] for s in steps]), ops=flat([s[0] for s in steps], 5, np.uint32),
        cand_first=first([s[1] for s in steps]), cands=flat([s[1] for s in steps], 4, np.int64),
        conn=np.array([s[2] for s in steps], np.int64), visit_first=first(visits), visits=flat(visits, 2, np.int64),
        active=np.array(active, np.uint8), tree_first=first(tree), tree=flat(tree, 3, np.uint32))
    print("%s: %d cases, %d steps, %d ops, %d visits; %d bytes" % (os.path.relpath(OUT, ROOT), len(C), len(steps),
                                                                  sum(len(s[0]) for s in steps), sum(map(len, visits)), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
