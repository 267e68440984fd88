/*
 * h2o's per-string symbols from many threads whose answers differ (include/hhuff.h (1), linked against
 * h2o_amd/libhhuff.so).  tests/encode_edges.py writes the files, tests/test_per_string_service.py runs this:
 *
 *   per_string_check MODE CASES PLAN [BATCH]
 *
 * CASES: the calls with their expected return value, bytes and soft_errors word.  PLAN: per thread the ordered list
 * of {case, microseconds to sleep before the call}.  BATCH: a decode batch with its expected results, for a thread of
 * kind 1, which runs hhuff_decode_batch on a stream of its own for as long as the calling threads work.
 *
 * The calling threads make their first call one after another in thread order, so thread number k of them owns
 * mailbox k mod 64 of the resident service (svc_call, hhuff_capi_string.hip).  With the plan's lock-step flag they then go
 * round by round, a barrier before every call, so that the requests of a round are posted together.  Every thread
 * checks every call itself: the return value, every output byte, the soft_errors word, the sentinel bytes of dst behind
 * the result and behind dst, and through hhuff_service_stamps whether the service's wave served the call -- it must
 * for an input of up to 768 bytes and must not for a longer one (MODE service), or must never (MODE launch, run with
 * HHUFF_NO_SERVICE=1).  The first mismatch of a thread is reported with thread, mailbox, round and the case's label.
 * MODE nogpu: every call of every thread must return SIZE_MAX with a reason in hhuff_last_error_string(), no abort.
 * Exit 0 and a line "per_string_check: ok ..." when every check held.
 */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <hip/hip_runtime_api.h>

#include "hhuff.h"

enum { MODE_SERVICE, MODE_LAUNCH, MODE_NOGPU };
enum { KIND_CALLS = 0, KIND_BATCH = 1, FLAG_LOOP = 1, GUARD = 64, SENTINEL = 0xA5, SVC_MAX = 768 };

typedef struct {
    uint32_t op, is_name, soft_in, in_len, out_len, soft, label_len, pad;
    uint64_t ret;
    char *label;
    uint8_t *in, *out;
} Case;

typedef struct {
    uint32_t kind, device, flags, n;
    uint32_t *idx, *sleep_us;
    int id, ordinal; /* ordinal: among the calling threads (the mailbox is ordinal mod 64) */
    pthread_t th;
    uint64_t calls, served, batches;
    int failed;
    char msg[640];
} Thread;

static int g_mode, g_lockstep;
static uint32_t g_ncases, g_nthreads, g_ncallers, g_nsteady;
static Case *g_cases;
static Thread *g_threads;
static uint8_t *g_batch;
static pthread_barrier_t g_barrier;
static pthread_mutex_t g_turn_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_turn_cv = PTHREAD_COND_INITIALIZER;
static int g_turn;
static atomic_int g_working; /* calling threads without FLAG_LOOP that are not done yet */

static uint8_t *read_file(const char *path, size_t *size)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    *size = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *p = malloc(*size + 1);
    if (fread(p, 1, *size, f) != *size)
        exit(2);
    fclose(f);
    return p;
}

static void load_cases(const char *path)
{
    size_t size;
    uint8_t *p = read_file(path, &size), *end = p + size;
    if (size < 8 || memcmp(p, "PSC1", 4) != 0)
        exit(2);
    memcpy(&g_ncases, p + 4, 4);
    g_cases = calloc(g_ncases ? g_ncases : 1, sizeof(Case));
    p += 8;
    for (uint32_t i = 0; i < g_ncases; ++i) {
        Case *c = &g_cases[i];
        if ((size_t)(end - p) < 40)
            exit(2);
        memcpy(c, p, 32);
        memcpy(&c->ret, p + 32, 8);
        p += 40;
        if ((size_t)(end - p) < (size_t)c->label_len + c->in_len + c->out_len)
            exit(2);
        c->label = malloc(c->label_len + 1);
        memcpy(c->label, p, c->label_len);
        c->label[c->label_len] = '\0';
        c->in = p + c->label_len;
        c->out = c->in + c->in_len;
        p = c->out + c->out_len;
    }
}

static void load_plan(const char *path)
{
    size_t size;
    uint8_t *p = read_file(path, &size), *end = p + size;
    if (size < 12 || memcmp(p, "PSP1", 4) != 0)
        exit(2);
    uint32_t lock;
    memcpy(&g_nthreads, p + 4, 4);
    memcpy(&lock, p + 8, 4);
    g_lockstep = (int)lock;
    g_threads = calloc(g_nthreads ? g_nthreads : 1, sizeof(Thread));
    p += 12;
    for (uint32_t t = 0; t < g_nthreads; ++t) {
        Thread *T = &g_threads[t];
        if ((size_t)(end - p) < 16)
            exit(2);
        memcpy(T, p, 16);
        p += 16;
        if ((size_t)(end - p) < 8 * (size_t)T->n)
            exit(2);
        T->idx = malloc(4 * (size_t)T->n + 4);
        T->sleep_us = malloc(4 * (size_t)T->n + 4);
        for (uint32_t k = 0; k < T->n; ++k, p += 8) {
            memcpy(&T->idx[k], p, 4);
            memcpy(&T->sleep_us[k], p + 4, 4);
            if (T->kind == KIND_CALLS && T->idx[k] >= g_ncases)
                exit(2);
        }
        T->id = (int)t;
        if (T->kind == KIND_CALLS) {
            T->ordinal = (int)g_ncallers++;
            if (!(T->flags & FLAG_LOOP))
                ++g_nsteady;
        }
    }
}

static int stamps(uint32_t out4[4])
{
    return g_mode == MODE_NOGPU ? HHUFF_EINVAL : hhuff_service_stamps(out4);
}

/* one call, checked: 0, or 1 with T->msg written */
static int one_call(Thread *T, uint32_t round, const Case *c, uint8_t *dst, size_t cap)
{
    const char *what = c->op ? "encode" : "decode";
    memset(dst, SENTINEL, cap + GUARD);
    uint32_t before[4] = {0, 0, 0, 0}, after[4] = {0, 0, 0, 0};
    const int rb = stamps(before);
    unsigned soft = c->soft_in;
    const size_t r = c->op ? h2o_hpack_encode_huffman(dst, c->in, c->in_len)
                           : h2o_hpack_decode_huffman((char *)dst, &soft, c->in, c->in_len, (int)c->is_name, NULL);
    int ra = stamps(after);
    ++T->calls;
#define FAIL(...)                                                                                                      \
    do {                                                                                                               \
        int n_ = snprintf(T->msg, sizeof(T->msg), "thread %d mailbox %d round %u case '%s' (%s, %u bytes): ", T->id,   \
                          T->ordinal % 64, round, c->label, what, c->in_len);                                          \
        snprintf(T->msg + n_, sizeof(T->msg) - (size_t)n_, __VA_ARGS__);                                               \
        return 1;                                                                                                      \
    } while (0)
    if (g_mode == MODE_NOGPU) {
        if (r != SIZE_MAX)
            FAIL("returned %zu without a GPU", r);
        if (hhuff_last_error_string()[0] == '\0')
            FAIL("SIZE_MAX without a reason in hhuff_last_error_string()");
        if (soft != c->soft_in)
            FAIL("soft_errors %#x after a failed call, was %#x", soft, c->soft_in);
        return 0;
    }
    if (r != (size_t)c->ret)
        FAIL("returned %zu, expected %zu (%s)", r, (size_t)c->ret, hhuff_last_error_string());
    if (!c->op && soft != c->soft)
        FAIL("soft_errors %#x, expected %#x (preset %#x)", soft, c->soft, c->soft_in);
    if (r != SIZE_MAX) {
        for (size_t i = 0; i < r; ++i)
            if (dst[i] != c->out[i])
                FAIL("output byte %zu of %zu is %#04x, expected %#04x", i, r, dst[i], c->out[i]);
        for (size_t i = r; i < cap; ++i)
            if (dst[i] != SENTINEL)
                FAIL("dst byte %zu behind the result of %zu bytes was written (%#04x)", i, r, dst[i]);
    }
    for (size_t i = cap; i < cap + GUARD; ++i)
        if (dst[i] != SENTINEL)
            FAIL("byte %zu behind dst (%zu bytes) was written (%#04x)", i - cap, cap, dst[i]);
    int changed = ra == HHUFF_OK && (rb != HHUFF_OK || memcmp(before, after, 16) != 0);
    if (g_mode == MODE_SERVICE && c->in_len <= SVC_MAX) {
        /* the wave stores the stamps just before the result: give that store a moment to show */
        for (int k = 0; k < 100000 && !changed; ++k) {
            ra = stamps(after);
            changed = ra == HHUFF_OK && (rb != HHUFF_OK || memcmp(before, after, 16) != 0);
        }
        if (!changed)
            FAIL("not served by the service (stamps rc %d -> %d, unchanged; %s)", rb, ra, hhuff_last_error_string());
        ++T->served;
    } else if (changed) {
        FAIL("served by the service (the stamps changed), expected the launch path");
    }
#undef FAIL
    return 0;
}

static void pause_us(uint32_t us)
{
    if (us) {
        struct timespec ts = {us / 1000000u, (long)(us % 1000000u) * 1000L};
        nanosleep(&ts, NULL);
    }
}

static void *caller(void *arg)
{
    Thread *T = arg;
    size_t cap = 0;
    for (uint32_t k = 0; k < T->n; ++k) {
        const Case *c = &g_cases[T->idx[k]];
        const size_t need = c->op ? c->in_len : 2 * (size_t)c->in_len;
        cap = need > cap ? need : cap;
    }
    uint8_t *dst = malloc(cap + GUARD + 1);
    if (g_mode != MODE_NOGPU && hipSetDevice((int)T->device) != hipSuccess) {
        snprintf(T->msg, sizeof(T->msg), "thread %d: hipSetDevice(%u) failed", T->id, T->device);
        T->failed = 1;
    }
    const int steady = !(T->flags & FLAG_LOOP);
    for (uint32_t lap = 0, round = 0;; ++lap) {
        for (uint32_t k = 0; k < T->n; ++k, ++round) {
            const Case *c = &g_cases[T->idx[k]];
            if (round == 0) { /* the first calls in thread order: the mailboxes are known */
                pthread_mutex_lock(&g_turn_mu);
                while (g_turn != T->ordinal)
                    pthread_cond_wait(&g_turn_cv, &g_turn_mu);
            } else if (g_lockstep && steady) {
                pthread_barrier_wait(&g_barrier);
            }
            pause_us(T->sleep_us[k]);
            if (!T->failed) /* (a thread that failed still keeps the others' barriers) */
                T->failed = one_call(T, round, c, dst, c->op ? c->in_len : 2 * (size_t)c->in_len);
            if (round == 0) {
                ++g_turn;
                pthread_cond_broadcast(&g_turn_cv);
                pthread_mutex_unlock(&g_turn_mu);
                if (g_lockstep && steady)
                    pthread_barrier_wait(&g_barrier);
            }
            if (!steady && round > 0 && atomic_load(&g_working) == 0)
                goto out;
        }
        if (steady || T->n == 0 || lap > 1000000u)
            break;
    }
out:
    if (steady)
        atomic_fetch_sub(&g_working, 1);
    if (!T->failed && g_mode != MODE_NOGPU && hhuff_last_error_string()[0] != '\0') {
        snprintf(T->msg, sizeof(T->msg), "thread %d mailbox %d: hhuff_last_error_string() is \"%s\" after %llu good calls",
                 T->id, T->ordinal % 64, hhuff_last_error_string(), (unsigned long long)T->calls);
        T->failed = 1;
    }
    free(dst);
    return NULL;
}

/* hhuff_decode_batch on a stream of this thread's, against the file's expected results, while the callers work */
static void *batcher(void *arg)
{
    Thread *T = arg;
    uint32_t n;
    uint64_t in_size, out_size;
    memcpy(&n, g_batch + 4, 4);
    memcpy(&in_size, g_batch + 8, 8);
    memcpy(&out_size, g_batch + 16, 8);
    const size_t nw = (n + 31) / 32, nst = ((size_t)n + 3) / 4 * 4;
    const uint8_t *p = g_batch + 24;
    const uint32_t *off = (const uint32_t *)p, *names = off + n + 1, *exp_len = names + nw;
    const uint8_t *exp_st = (const uint8_t *)(exp_len + n), *in = exp_st + nst, *exp_out = in + in_size;
    uint8_t *d_in = NULL, *d_out = NULL, *d_st = NULL, *out = malloc(out_size + 1), *st = malloc(n + 1);
    uint32_t *d_off = NULL, *d_names = NULL, *d_len = NULL, *len = malloc(4 * (size_t)n + 4);
    hipStream_t s = NULL;
#define BFAIL(...)                                                                                                     \
    do {                                                                                                               \
        int n_ = snprintf(T->msg, sizeof(T->msg), "thread %d (batch) pass %llu: ", T->id, (unsigned long long)T->batches); \
        snprintf(T->msg + n_, sizeof(T->msg) - (size_t)n_, __VA_ARGS__);                                               \
        T->failed = 1;                                                                                                 \
        goto done;                                                                                                     \
    } while (0)
    if (hipSetDevice((int)T->device) || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) ||
        hipMalloc((void **)&d_in, in_size + 16) || hipMalloc((void **)&d_out, out_size + 16) ||
        hipMalloc((void **)&d_off, 4 * ((size_t)n + 1)) || hipMalloc((void **)&d_names, 4 * nw + 4) ||
        hipMalloc((void **)&d_len, 4 * (size_t)n + 4) || hipMalloc((void **)&d_st, n + 4) ||
        hipMemcpy(d_in, in, in_size, hipMemcpyHostToDevice) ||
        hipMemcpy(d_off, off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice) ||
        hipMemcpy(d_names, names, 4 * nw, hipMemcpyHostToDevice))
        BFAIL("HIP setup failed");
    do {
        if (hipMemsetAsync(d_out, 0, out_size, s) || hipMemsetAsync(d_len, 0xEE, 4 * (size_t)n, s) ||
            hipMemsetAsync(d_st, 0xEE, n, s))
            BFAIL("hipMemsetAsync failed");
        const int rc = hhuff_decode_batch(d_in, in_size, d_off, NULL, n, d_names, d_out, NULL, d_len, d_st, s);
        if (rc != HHUFF_OK)
            BFAIL("hhuff_decode_batch returned %d (%s)", rc, hhuff_last_error_string());
        if (hipMemcpyAsync(out, d_out, out_size, hipMemcpyDeviceToHost, s) ||
            hipMemcpyAsync(len, d_len, 4 * (size_t)n, hipMemcpyDeviceToHost, s) ||
            hipMemcpyAsync(st, d_st, n, hipMemcpyDeviceToHost, s) || hipStreamSynchronize(s))
            BFAIL("copy back failed");
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t at = ((uint64_t)off[i] * 8) / 5;
            if (len[i] != exp_len[i] || st[i] != exp_st[i])
                BFAIL("string %u: out_len %#x status %#x, expected %#x %#x", i, len[i], st[i], exp_len[i], exp_st[i]);
            if (len[i] != HHUFF_FAIL_LEN && memcmp(out + at, exp_out + at, len[i]) != 0)
                BFAIL("string %u: decoded bytes differ", i);
        }
        ++T->batches;
    } while (atomic_load(&g_working) > 0 && T->batches < 100000);
done:
#undef BFAIL
    hipFree(d_in), hipFree(d_out), hipFree(d_off), hipFree(d_names), hipFree(d_len), hipFree(d_st);
    if (s)
        hipStreamDestroy(s);
    free(out), free(st), free(len);
    return NULL;
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s service|launch|nogpu CASES PLAN [BATCH]\n", argv[0]);
        return 2;
    }
    g_mode = strcmp(argv[1], "nogpu") == 0 ? MODE_NOGPU : strcmp(argv[1], "launch") == 0 ? MODE_LAUNCH : MODE_SERVICE;
    load_cases(argv[2]);
    load_plan(argv[3]);
    if (argc > 4) {
        size_t size;
        g_batch = read_file(argv[4], &size);
        if (size < 24 || memcmp(g_batch, "PSB1", 4) != 0)
            return 2;
    }
    atomic_store(&g_working, (int)g_nsteady);
    pthread_barrier_init(&g_barrier, NULL, g_nsteady ? g_nsteady : 1);
    for (uint32_t t = 0; t < g_nthreads; ++t) {
        Thread *T = &g_threads[t];
        if (T->kind == KIND_BATCH && (!g_batch || g_mode == MODE_NOGPU))
            continue;
        pthread_create(&T->th, NULL, T->kind == KIND_BATCH ? batcher : caller, T);
    }
    int fail = 0;
    uint64_t calls = 0, served = 0, batches = 0;
    for (uint32_t t = 0; t < g_nthreads; ++t) {
        Thread *T = &g_threads[t];
        if (T->kind == KIND_BATCH && (!g_batch || g_mode == MODE_NOGPU))
            continue;
        pthread_join(T->th, NULL);
        calls += T->calls, served += T->served, batches += T->batches;
        if (T->failed) {
            fprintf(stderr, "%s\n", T->msg);
            fail = 1;
        }
    }
    printf("per_string_check: %s threads=%u calls=%llu served=%llu batches=%llu\n", fail ? "FAILED" : "ok", g_nthreads,
           (unsigned long long)calls, (unsigned long long)served, (unsigned long long)batches);
    return fail;
}
