/*
 * uaes_engine.c -- host layer of the MI355X AES engine (plain C).
 *
 * Mirrors the mode drivers of the reference (AES_ECB_*, AES_CTR_*, AES_XTS_*,
 * AES_GCM_*; micro_aes.c:636-680, :962-990, :1066-1093, :1164-1212): argument
 * checking, the reference's error behaviour, the key schedule
 * (KeyExpansion, micro_aes.c:144-178 -- host side, <= 240 bytes of output),
 * and buffer plumbing.  ALL block-cipher and GHASH work happens in the HIP
 * kernels behind uaes_device.h; there is no CPU data path here to fall back
 * to, and a missing/failed HIP device is reported, never papered over.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/uaes_hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"
#include "uaes_host.h"

#define UAES_VERSION "uaes-hip 0.1 gfx950"
#define MAX_DEVICES  16

/* ------------------------------------------------------------------------ */
/* errors                                                                     */
/* ------------------------------------------------------------------------ */
static __thread char tls_err[256];

static int g_device_suspect;                       /* set by every UAES_E_HIP: the host fallback looks at the device again */
static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tls_err, sizeof tls_err, fmt, ap);
    va_end(ap);
    if (code == UAES_E_HIP) __atomic_store_n(&g_device_suspect, 1, __ATOMIC_RELEASE);
    return code;
}

#define HIPCHK(call)                                                               \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess)                                                      \
            return fail(UAES_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define KCHK(call)                                                                        \
    do {                                                                                  \
        int e_ = (call);                                                                  \
        if (e_ != 0)                                                                      \
            return fail(UAES_E_HIP, "%s failed: %s", #call, hipGetErrorString((hipError_t)e_)); \
    } while (0)

const char *uaes_last_error(void) { return tls_err; }
const char *uaes_version(void) { return UAES_VERSION; }

/* ------------------------------------------------------------------------ */
/* policy switch: what a failed authentication leaves in the caller's buffer   */
/* ------------------------------------------------------------------------ */
/* The reference's default build decrypts CCM / GCM-SIV / OCB BEFORE it authenticates and its
 * SABOTAGE() is a no-op (micro_aes.c:1306-1312, :1500-1511, :1803-1810), so a forged message
 * leaves attacker-chosen plaintext in pntxt next to the 0x1A; with INCREASE_SECURITY it wipes
 * the buffer.  Default here = the reference's default (bit-identical behaviour); switching
 * this on gives the INCREASE_SECURITY behaviour: on 0x1A the output is all zero bytes.
 * (GCM never releases unauthenticated text in either build: N7.)                          */
static int g_wipe_on_auth_failure = 0;

int uaes_set_wipe_on_auth_failure(int on)
{
    return __atomic_exchange_n(&g_wipe_on_auth_failure, on != 0, __ATOMIC_ACQ_REL);
}

static int wipe_on_auth_failure(void) { return __atomic_load_n(&g_wipe_on_auth_failure, __ATOMIC_ACQUIRE); }
/* GCM decrypt into the caller's device buffer: two passes (tag first, N7) unless the caller has
 * accepted a zeroed output on failure, which lets CTR and GHASH share one pass (uaesk_gcm, mode 2) */
/* GCM decryption into a caller's DEVICE buffer: two passes (GHASH, tag check, then CTR -- nothing is written
 * before the tag is known, N7) unless the caller has asked for the one-pass order BY NAME: the text is then written
 * while it is hashed and zeroed if the tag turns out wrong.  (Round 2 hung this on the wipe switch above, whose name
 * promises more safety, not less: ADVICE r02.)                                                              */
static int g_gcm_one_pass = 0;

int uaes_set_gcm_one_pass_decrypt(int on)
{
    return __atomic_exchange_n(&g_gcm_one_pass, on != 0, __ATOMIC_ACQ_REL);
}

static int gcm_decrypt_mode(void) { return __atomic_load_n(&g_gcm_one_pass, __ATOMIC_ACQUIRE) ? 2 : 1; }

/* tag comparison whose run time does not depend on where the tags differ */
static int tags_differ(const uint8_t *a, const uint8_t *b, size_t n)
{
    unsigned acc = 0;
    size_t i;
    for (i = 0; i < n; ++i) acc |= (unsigned)(a[i] ^ b[i]);
    return acc != 0;
}

/* ------------------------------------------------------------------------ */
/* S-box and lookup-table generation (FIPS-197 sec. 5.1.1 / 5.3.2).            */
/* Built once from the field arithmetic with log/antilog tables over the      */
/* generator 0x03, then uploaded to every device context.                     */
/* ------------------------------------------------------------------------ */
static uint8_t  h_sbox[256], h_isbox[256];
static uint32_t h_te0[256], h_td0[256];
static pthread_once_t tables_once = PTHREAD_ONCE_INIT;

static uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a >> 7) * 0x1b)); }

/* Frobenius matrices of GHASH's field (uaesk_tables.frob): rows of x -> x^(2^k), k = 1..63.
 * Element = (hi, lo), coefficient of x^q at bit 127-q (hi bit 63 = x^0); times x = shift right,
 * the bit falling off re-enters as 0xE1 << 120 (SP 800-38D; mulGF128, micro_aes.c:476-493).   */
#define FROB_K 63
static uint64_t h_frob[FROB_K * 256];

static void gf128_mul(const uint64_t a[2], const uint64_t b[2], uint64_t z[2])
{
    uint64_t vh = b[0], vl = b[1], zh = 0, zl = 0;
    int q;
    for (q = 0; q < 128; ++q) {
        const uint64_t bit = q < 64 ? (a[0] >> (63 - q)) & 1 : (a[1] >> (127 - q)) & 1;
        const uint64_t m = 0 - bit, carry = vl & 1;
        zh ^= vh & m;
        zl ^= vl & m;
        vl = (vl >> 1) | (vh << 63);
        vh = (vh >> 1) ^ (carry ? 0xE100000000000000ull : 0);
    }
    z[0] = zh; z[1] = zl;
}

static void build_frobenius(void)
{
    static uint64_t col[128][2];           /* image of basis bit j (position j: < 64 = hi bit j, else lo bit j-64) */
    int j, k, p;
    for (j = 0; j < 128; ++j) { col[j][0] = j < 64 ? 1ull << j : 0; col[j][1] = j < 64 ? 0 : 1ull << (j - 64); }
    for (k = 1; k <= FROB_K; ++k) {
        uint64_t *rows = h_frob + (size_t)(k - 1) * 256;
        for (j = 0; j < 128; ++j) {
            uint64_t sq[2];
            gf128_mul(col[j], col[j], sq);
            col[j][0] = sq[0]; col[j][1] = sq[1];
        }
        memset(rows, 0, 256 * sizeof *rows);
        for (j = 0; j < 128; ++j)
            for (p = 0; p < 128; ++p)
                if ((p < 64 ? col[j][0] >> p : col[j][1] >> (p - 64)) & 1)
                    rows[2 * p + (j >= 64)] |= 1ull << (j & 63);
    }
}

static void build_host_tables(void)
{
    uint8_t alog[256], logt[256];
    uint8_t a = 1;
    int i;
    for (i = 0; i < 255; ++i) {                 /* powers of the generator 3   */
        alog[i] = a;
        logt[a] = (uint8_t)i;
        a = (uint8_t)(a ^ xtime(a));
    }
    alog[255] = alog[0];
    for (i = 0; i < 256; ++i) {
        uint8_t inv = i ? alog[(255 - logt[i]) % 255] : 0, s = inv, r = inv;
        int k;
        for (k = 0; k < 4; ++k) {               /* affine map: xor of 4 rotations + 0x63 */
            r = (uint8_t)((r << 1) | (r >> 7));
            s ^= r;
        }
        s ^= 0x63;
        h_sbox[i] = s;
        h_isbox[s] = (uint8_t)i;
    }
    for (i = 0; i < 256; ++i) {
        uint8_t s = h_sbox[i], s2 = xtime(s), s3 = (uint8_t)(s2 ^ s);
        uint8_t v = h_isbox[i], v2 = xtime(v), v4 = xtime(v2), v8 = xtime(v4);
        uint8_t v9 = (uint8_t)(v8 ^ v), vb = (uint8_t)(v8 ^ v2 ^ v);
        uint8_t vd = (uint8_t)(v8 ^ v4 ^ v), ve = (uint8_t)(v8 ^ v4 ^ v2);
        h_te0[i] = (uint32_t)s2 | ((uint32_t)s << 8) | ((uint32_t)s << 16) | ((uint32_t)s3 << 24);
        h_td0[i] = (uint32_t)ve | ((uint32_t)v9 << 8) | ((uint32_t)vd << 16) | ((uint32_t)vb << 24);
    }
    build_frobenius();
    uaesh_tables_init(h_te0, h_td0);               /* the host data path's tables (uaes_host.c): off unless switched on */
}

/* ------------------------------------------------------------------------ */
/* key schedule: KeyExpansion (micro_aes.c:144-178) on little-endian words,   */
/* plus the equivalent-inverse-cipher keys (FIPS-197 sec. 5.3.5) for the      */
/* table-driven decrypt kernels.                                              */
/* ------------------------------------------------------------------------ */
typedef struct {
    int      nr;
    uaesk_rk ek, dk;
} keysched;

static uint32_t subword(uint32_t w)
{
    return (uint32_t)h_sbox[w & 0xff] | ((uint32_t)h_sbox[(w >> 8) & 0xff] << 8) |
           ((uint32_t)h_sbox[(w >> 16) & 0xff] << 16) | ((uint32_t)h_sbox[w >> 24] << 24);
}

static uint32_t inv_mix_word(uint32_t w)
{
    /* InvMixColumns of one column = xor of Td0-rotations of S(byte): undo the
     * S-box that Td0 applies by indexing with sbox[]                          */
    uint32_t r = 0;
    int b;
    for (b = 0; b < 4; ++b) {
        uint32_t t = h_td0[h_sbox[(w >> (8 * b)) & 0xff]];
        r ^= (t << (8 * b)) | (b ? t >> (32 - 8 * b) : 0);
    }
    return r;
}

static int expand_key(keysched *ks, const uint8_t *key, int keybits)
{
    int nk, total, i;
    uint8_t rcon = 1;
    if (keybits != 128 && keybits != 192 && keybits != 256)
        return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if (!key) return fail(UAES_E_ARG, "NULL key");
    pthread_once(&tables_once, build_host_tables);
    nk = keybits / 32;
    ks->nr = nk + 6;
    total = 4 * (ks->nr + 1);
    memset(&ks->ek, 0, sizeof ks->ek);
    memset(&ks->dk, 0, sizeof ks->dk);
    memcpy(ks->ek.w, key, (size_t)(4 * nk));     /* LE words of the byte stream */
    for (i = nk; i < total; ++i) {
        uint32_t t = ks->ek.w[i - 1];
        if (i % nk == 0) {
            t = subword((t >> 8) | (t << 24)) ^ rcon;      /* RotWord on LE words */
            rcon = xtime(rcon);
        } else if (nk == 8 && i % nk == 4) {
            t = subword(t);
        }
        ks->ek.w[i] = ks->ek.w[i - nk] ^ t;
    }
    for (i = 0; i < 4; ++i) {
        ks->dk.w[i] = ks->ek.w[4 * ks->nr + i];
        ks->dk.w[4 * ks->nr + i] = ks->ek.w[i];
    }
    for (i = 1; i < ks->nr; ++i) {
        int c;
        for (c = 0; c < 4; ++c)
            ks->dk.w[4 * i + c] = inv_mix_word(ks->ek.w[4 * (ks->nr - i) + c]);
    }
    return 0;
}

/* diagnostic export: lets the CPU test-suite check the schedule without a GPU */
int uaes_expand_key(int keybits, const uint8_t *key, uint32_t enc_words[60], uint32_t dec_words[60])
{
    keysched ks;
    int rc = expand_key(&ks, key, keybits);
    if (rc) return rc;
    if (enc_words) memcpy(enc_words, ks.ek.w, sizeof ks.ek.w);
    if (dec_words) memcpy(dec_words, ks.dk.w, sizeof ks.dk.w);
    return ks.nr;
}

/* ------------------------------------------------------------------------ */
/* per-device context                                                         */
/* ------------------------------------------------------------------------ */
/* Device scratch (GHASH tables and accumulators, XTS chunk tweaks, OCB offsets) is private
 * to the stream a call is enqueued on: work on one stream is ordered, work on different
 * streams may overlap, so several *_dev calls can be in flight per device.             */
#define SCRATCH_SLOTS 8

struct lane;

typedef struct {
    int             ready, sync_made;
    uaesk_tables    tb;
    void           *d_tables;
    struct {
        void  *stream;              /* hipStream_t the slot belongs to (NULL = default stream) */
        int    used;
        int    pins;                /* callers between "got this buffer" and "launch issued"   */
        unsigned long tick;         /* last use, for LRU recycling                             */
        void  *buf;
        size_t cap;
    } slot[SCRATCH_SLOTS];          /* scratch of the *_dev API, one per caller stream         */
    unsigned long   tick;
    pthread_cond_t  cv;             /* signalled when a pin is dropped / the pipeline is free  */
    struct {                        /* slice pipeline for long host texts: one entry per worker thread */
        void  *stream;
        void  *dbuf;                /* device slice                                            */
        void  *xscratch;            /* the worker's own XTS chunk-tweak scratch                */
        size_t xscratch_cap;
    } pipe[16];
    int             pipe_busy;      /* a pipelined call owns pipe[] (c->mu is dropped while its workers run) */
    void           *spool[8];       /* wiped scratch buffers of finished GCM streams, for the next uaes_gcm_stream_begin:
                                     * hipMalloc + hipDeviceSynchronize + hipFree were 230 us of every streamed message */
    int             nspool;
    struct lane    *lanes;          /* every thread's lane on this device (uaes_shutdown)      */
    pthread_mutex_t mu;             /* slot[], pipe[] ownership, the lane list -- never held while the GPU works */
} context;

static context g_ctx[MAX_DEVICES];
static pthread_mutex_t g_init_mu = PTHREAD_MUTEX_INITIALIZER;

static int get_context(context **out)
{
    int dev = 0, n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(UAES_E_HIP, "no usable HIP device (%s); this library has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return fail(UAES_E_HIP, "device index %d out of range", dev);
    context *c = &g_ctx[dev];
    if (!c->ready) {
        pthread_mutex_lock(&g_init_mu);
        if (!c->ready) {
            hipError_t err;
            pthread_once(&tables_once, build_host_tables);
            err = hipMalloc(&c->d_tables, 4096 + sizeof h_frob);
            if (err == hipSuccess) err = hipMemcpy(c->d_tables, h_te0, 1024, hipMemcpyHostToDevice);
            if (err == hipSuccess) err = hipMemcpy((char *)c->d_tables + 1024, h_td0, 1024, hipMemcpyHostToDevice);
            if (err == hipSuccess) err = hipMemcpy((char *)c->d_tables + 4096, h_frob, sizeof h_frob, hipMemcpyHostToDevice);
            if (err != hipSuccess) {
                pthread_mutex_unlock(&g_init_mu);
                return fail(UAES_E_HIP, "context setup failed: %s", hipGetErrorString(err));
            }
            c->tb.te0 = (const uint32_t *)c->d_tables;
            c->tb.td0 = (const uint32_t *)((char *)c->d_tables + 1024);
            c->tb.frob = (const uint64_t *)((char *)c->d_tables + 4096);
            if (!c->sync_made) {                   /* survives uaes_shutdown(): lanes keep pointing at it */
                pthread_mutex_init(&c->mu, NULL);
                pthread_cond_init(&c->cv, NULL);
                c->sync_made = 1;
            }
            uaesk_device_info(NULL, NULL);
            __atomic_store_n(&c->ready, 1, __ATOMIC_RELEASE);
        }
        pthread_mutex_unlock(&g_init_mu);
    }
    *out = c;
    return 0;
}

static int grow_on(void *stream, void **buf, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    if (*buf) {
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));  /* the only stream that ever used this buffer */
        HIPCHK(hipFree(*buf));
        *buf = NULL;
        *cap = 0;
    }
    need = (need + (1u << 20)) & ~(((size_t)1 << 20) - 1);
    HIPCHK(hipMalloc(buf, need));
    *cap = need;
    return 0;
}

/* The last SCRATCH_TAIL bytes of a scratch buffer (lanes, *_dev slots) are words that are ZERO BETWEEN CALLS: the
 * workgroups of a one-launch call count themselves in on one and the last arrival puts the zero back (uaesk_ocb's
 * done_word).  Cleared when the buffer is allocated, on the stream that uses it; no kernel's scratch layout
 * reaches them (every request is made SCRATCH_TAIL bytes larger).                                            */
#define SCRATCH_TAIL 256u
static unsigned *scratch_done_word(void *buf, size_t cap)
{
    return (unsigned *)((char *)buf + cap - SCRATCH_TAIL);
}

/* The word the calling thread armed last (arm_done_word) and the stream its call ran on.  The workgroups of a
 * one-launch call restore the zero themselves; a call that did NOT run to its end -- a launch the runtime refused, a
 * sequence abandoned half-way -- may not have, and a count left behind would make the next call on that word fold too
 * early.  Every failure path therefore puts the zero back, in stream order behind whatever did get queued
 * (lane_abandon, and any non-zero launch rc). */
static __thread unsigned *tls_armed_word;
static void arm_done_word(unsigned *w)
{
    if (w) tls_armed_word = w;
    uaesk_done_word_arm(w);
}
static void repair_done_word(void *stream)
{
    if (tls_armed_word) (void)hipMemsetAsync(tls_armed_word, 0, SCRATCH_TAIL, (hipStream_t)stream);
    tls_armed_word = NULL;
}
/* the *_dev calls: one kernel-level call on the caller's stream, nothing else can fail afterwards */
static void disarm_done_word_dev(void *stream, int launch_rc)
{
    uaesk_done_word_arm(NULL);
    if (launch_rc != 0) repair_done_word(stream);
    tls_armed_word = NULL;
}

/* for buffers that several streams may have used (the *_dev scratch slots) */
static int grow(void **buf, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    if (*buf) HIPCHK(hipDeviceSynchronize());
    return grow_on(NULL, buf, cap, need);
}

/* Scratch of at least `need` bytes for work about to be enqueued on `stream`; the caller
 * holds c->mu.  The slot comes back PINNED: until scratch_unpin() it is never recycled for
 * another stream, regrown or freed, so a *_dev caller may drop c->mu, enqueue its kernels and
 * unpin afterwards.  Once the launch is issued the buffer is protected by stream order and by
 * the hipDeviceSynchronize() that precedes every recycling / regrowing.  With all slots taken
 * the least recently used unpinned one is recycled; uaes_stream_release() gives a slot back.
 * (Only the *_dev API uses these slots: the synchronous API works on per-thread lanes and the
 * slice pipeline on its workers' own buffers, so neither can push a caller's stream out.)   */
static int scratch_pin(context *c, void *stream, size_t need, void **buf, int *slot_out)
{
    for (;;) {
        int i, k = -1;
        for (i = 0; i < SCRATCH_SLOTS && k < 0; ++i)
            if (c->slot[i].used && c->slot[i].stream == stream) k = i;
        for (i = 0; i < SCRATCH_SLOTS && k < 0; ++i)
            if (!c->slot[i].used) k = i;
        if (k < 0) {                              /* all taken: recycle the LRU slot nobody is about to use */
            for (i = 0; i < SCRATCH_SLOTS; ++i)
                if (c->slot[i].pins == 0 && (k < 0 || c->slot[i].tick < c->slot[k].tick)) k = i;
            if (k < 0) { pthread_cond_wait(&c->cv, &c->mu); continue; }
            HIPCHK(hipDeviceSynchronize());       /* everything already issued on the old stream is done */
            c->slot[k].stream = stream;
        }
        if (need + SCRATCH_TAIL > c->slot[k].cap && c->slot[k].pins > 0) {
            pthread_cond_wait(&c->cv, &c->mu);    /* another caller of this stream is about to launch on it */
            continue;
        }
        c->slot[k].used = 1;
        c->slot[k].stream = stream;
        c->slot[k].tick = ++c->tick;
        {
            const size_t before = c->slot[k].cap;
            if (grow(&c->slot[k].buf, &c->slot[k].cap, need + SCRATCH_TAIL)) return UAES_E_HIP;
            if (c->slot[k].cap != before)
                HIPCHK(hipMemsetAsync(scratch_done_word(c->slot[k].buf, c->slot[k].cap), 0, SCRATCH_TAIL, (hipStream_t)stream));
        }
        c->slot[k].pins++;
        *buf = c->slot[k].buf;
        *slot_out = k;
        return 0;
    }
}

static void scratch_unpin(context *c, int k)
{
    pthread_mutex_lock(&c->mu);
    if (k >= 0 && c->slot[k].pins > 0) {
        c->slot[k].pins--;
        pthread_cond_broadcast(&c->cv);
    }
    pthread_mutex_unlock(&c->mu);
}

/* ------------------------------------------------------------------------ */
/* lanes: what a host thread needs to run a SYNCHRONOUS call on its own        */
/* ------------------------------------------------------------------------ */
/* The reference keeps one global RoundKey (micro_aes.c:72) and cannot be called from two threads
 * at once.  Here every host thread that uses the synchronous (drop-in) API gets a LANE per
 * device: its own non-blocking stream, device staging buffers, pinned bounce buffers, GHASH /
 * XTS / OCB scratch and status words.  A call touches nothing but its thread's lane and read-only
 * context data, so N threads run N calls concurrently -- copies and kernels of different threads
 * overlap on the GPU -- and no lock is held while the GPU works.  A lane lives until its thread
 * exits (pthread key destructor) or uaes_shutdown().                                          */
typedef struct lane {
    context    *c;
    int         device;
    void       *stream;             /* hipStream_t, hipStreamNonBlocking                         */
    void       *stage[2];           /* device staging of host / misaligned texts                  */
    size_t      stage_cap[2];
    void       *scratch;            /* GHASH tables + accumulators, XTS chunk tweaks, OCB offsets */
    size_t      scratch_cap;
    void       *aad_stage;
    size_t      aad_cap;
    void       *pin[2];             /* pinned bounce buffers for short host texts (in, out)       */
    void       *pinx;               /* 4 KiB of pinned memory for small values exchanged mid-call;
                                     * its last 128 bytes: the completion ticket (lane_sync)       */
    uint32_t    seq;                /* number of the last ticket issued                            */
    uint32_t    armed;              /* != 0: the call's only kernel carries this ticket itself     */
    int        *d_status;           /* device: status word, and a 16-byte result slot at +4 ints  */
    /* The GCM key this thread used last on this device (lane_gcm_keyed): a caller of the drop-in API sends message
     * after message under one key, and the reference redoes GCMsetup for each (micro_aes.c:1140-1152).  The eighth
     * call in a row with the same key builds the key's whole table set in the lane's scratch once (what
     * uaes_gcm_key_new does), the following ones run as calls on a key context: only Enc(J0) per message.         */
    uint8_t     gk[32];
    int         gk_bits;
    int         gk_state;           /* 0 nothing, n < GK_BUILD_AT: calls in a row under this key, GK_TABLES: its tables are in `scratch` */
    struct lane *next;              /* context's list                                             */
} lane;

/* anything else that writes the lane's scratch (XTS chunk tweaks, OCB rows, GHASH under a foreign H ...) */
static void lane_scratch_clobbered(lane *L)
{
    L->gk_state = 0;
    memset(L->gk, 0, sizeof L->gk);
}

static __thread lane *tls_lane[MAX_DEVICES];
static pthread_key_t   lane_key;
static pthread_once_t  lane_key_once = PTHREAD_ONCE_INIT;

static void lane_free_resources(lane *L)
{
    int i;
    if (L->stream) (void)hipStreamSynchronize((hipStream_t)L->stream);
    for (i = 0; i < 2; ++i) {
        if (L->stage[i]) (void)hipFree(L->stage[i]);
        if (L->pin[i]) (void)hipHostFree(L->pin[i]);
    }
    if (L->pinx) (void)hipHostFree(L->pinx);
    if (L->scratch) {                             /* GHASH tables of H are key material */
        (void)hipMemset(L->scratch, 0, L->scratch_cap);
        (void)hipFree(L->scratch);
    }
    lane_scratch_clobbered(L);
    if (L->aad_stage) (void)hipFree(L->aad_stage);
    if (L->d_status) (void)hipFree(L->d_status);
    if (L->stream) (void)hipStreamDestroy((hipStream_t)L->stream);
    (void)hipGetLastError();
    L->stream = NULL; L->stage[0] = L->stage[1] = NULL; L->stage_cap[0] = L->stage_cap[1] = 0;
    L->pin[0] = L->pin[1] = NULL; L->pinx = NULL; L->scratch = NULL; L->scratch_cap = 0;
    L->aad_stage = NULL; L->aad_cap = 0; L->d_status = NULL;
}

static void lane_unlink(lane *L)
{
    lane **pp;
    pthread_mutex_lock(&L->c->mu);
    for (pp = &L->c->lanes; *pp; pp = &(*pp)->next)
        if (*pp == L) { *pp = L->next; break; }
    pthread_mutex_unlock(&L->c->mu);
}

/* a thread that used the library exits: give its lanes back */
static void lanes_of_thread_exit(void *unused)
{
    int d, prev = -1;
    (void)unused;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    for (d = 0; d < MAX_DEVICES; ++d) {
        lane *L = tls_lane[d];
        if (!L) continue;
        tls_lane[d] = NULL;
        if (hipSetDevice(L->device) == hipSuccess) {
            lane_unlink(L);
            lane_free_resources(L);
        }
        free(L);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}

static void lane_key_make(void) { (void)pthread_key_create(&lane_key, lanes_of_thread_exit); }

static int get_lane(context *c, lane **out)
{
    const int dev = (int)(c - g_ctx);
    lane *L = tls_lane[dev];
    if (!L) {
        pthread_once(&lane_key_once, lane_key_make);
        if ((L = (lane *)calloc(1, sizeof *L)) == NULL) return fail(UAES_E_HIP, "out of host memory");
        L->c = c;
        L->device = dev;
        pthread_mutex_lock(&c->mu);
        L->next = c->lanes;
        c->lanes = L;
        pthread_mutex_unlock(&c->mu);
        tls_lane[dev] = L;
        (void)pthread_setspecific(lane_key, (void *)1);   /* arms the exit destructor for this thread */
    }
    if (!L->stream) {                             /* new, or emptied by uaes_shutdown() */
        hipError_t e = hipStreamCreateWithFlags((hipStream_t *)&L->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc((void **)&L->d_status, 128);      /* [16]: workgroup count of a riding ticket */
        if (e == hipSuccess) e = hipMemset(L->d_status, 0, 128);
        if (e != hipSuccess) {
            if (L->stream) (void)hipStreamDestroy((hipStream_t)L->stream);
            L->stream = NULL;
            L->d_status = NULL;
            return fail(UAES_E_HIP, "lane setup failed: %s", hipGetErrorString(e));
        }
    }
    *out = L;
    return 0;
}

/* context + the calling thread's lane on the current device */
static int enter(context **c, lane **L)
{
    int rc = get_context(c);
    return rc ? rc : get_lane(*c, L);
}

/* The lane's scratch, for `owner`.  SCRATCH_GCM_KEYED: a GCM call under the lane's cached key -- the only user that
 * leaves the key's tables valid (lane_gcm_keyed decides whether they are there).  Anybody else (XTS chunk tweaks, OCB
 * rows, GHASH under a foreign H, GCM-SIV, a GCM shard ...) is about to overwrite them: asking for the buffer IS the
 * invalidation, no writer has to remember a second call. */
enum { SCRATCH_OTHER = 0, SCRATCH_GCM_KEYED = 1 };
static int lane_scratch(lane *L, size_t need, int owner)
{
    const size_t before = L->scratch_cap;
    if (owner != SCRATCH_GCM_KEYED) lane_scratch_clobbered(L);
    int rc = grow_on(L->stream, &L->scratch, &L->scratch_cap, need + SCRATCH_TAIL);
    if (rc) return rc;
    if (L->scratch_cap != before) {
        lane_scratch_clobbered(L);
        HIPCHK(hipMemsetAsync(scratch_done_word(L->scratch, L->scratch_cap), 0, SCRATCH_TAIL, (hipStream_t)L->stream));
    }
    return 0;
}

static int pinned_ready(lane *L);
static int env_int(const char *name, int dflt, int lo, int hi);

/* ---- waiting for the lane's stream ------------------------------------------------------------
 * hipStreamSynchronize costs ~11 us for an empty kernel and all host threads together get ~0.31 M of them per
 * second out of the runtime (tools/ubench/threadfloor.hip).  A synchronous call therefore ends with a TICKET: a
 * one-wave kernel behind the call's kernels stores the lane's next sequence number into pinned memory and the host
 * spins on that word (8.9 us, 0.6 M calls/s at 8 threads); the same kernel carries the few result bytes a call
 * reads back (status word, tag, MAC), which saves the hipMemcpyAsync command as well.  A call that is still running
 * after TICKET_SPIN_US (a long text, a hung or faulted kernel) goes into hipStreamSynchronize after all, which also
 * is where a device error surfaces.  UAES_TICKET=0 switches the mechanism off.                          */
#define TICKET_OFF      (4096 - 128)             /* byte offset of the ticket word in pinx   */
#define TICKET_DATA_OFF (4096 - 64)              /* 64 bytes of fetched result behind it     */
#define TICKET_SPIN_US  200
#define TICKET_RIDE_MAX_KIB 512                /* profiles/r05_ticket_ride_sweep.log: equal at 256-512 KiB, riding loses 1-8 us from 1 MiB on */

/* every setting read from the environment, once per process and race-free (the lazily initialised
 * function-local statics were a benign but real data race between the first calls of two threads) */
static struct {
    int    ticket, pipe_workers, gcm_key_cache;
    size_t ticket_ride_max;         /* longest text whose only kernel carries the completion ticket itself */
    size_t pin_bytes, zero_copy_max, pipe_slice;
} g_env;
static pthread_once_t g_env_once = PTHREAD_ONCE_INIT;
static void env_init(void);
static inline void env_ready(void) { (void)pthread_once(&g_env_once, env_init); }

static int ticket_enabled(void)
{
    env_ready();
    return g_env.ticket;
}

static int64_t now_us(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (int64_t)t.tv_sec * 1000000 + t.tv_nsec / 1000;
}

static volatile uint32_t *ticket_word(lane *L) { return (volatile uint32_t *)((char *)L->pinx + TICKET_OFF); }

static uint32_t ticket_next(lane *L)
{
    if (++L->seq == 0) ++L->seq;                              /* never 0: the page starts zeroed */
    return L->seq;
}

/* spin on the lane's ticket word until it shows seq; a call that takes longer sleeps in the runtime */
static int ticket_wait(lane *L, uint32_t seq)
{
    volatile uint32_t *flag = ticket_word(L);
    const int64_t t0 = now_us();
    unsigned spins = 0;
    for (;;) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return 0;
        __builtin_ia32_pause();
        if ((++spins & 255u) == 0 && now_us() - t0 > TICKET_SPIN_US) break;
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)L->stream));
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return fail(UAES_E_HIP, "completion ticket lost");
    return 0;
}

/* Right before a kernel-level call whose only (or last) launch may carry the ticket itself (uaes_device.h:
 * uaesk_ticket_arm) -- ECB, the generic CTR kernel, a one-launch XTS unit, a one-launch GCM encryption -- and right
 * after it: L->armed != 0 then says that the kernel releases that number and no ticket kernel is needed.       */
static void ticket_arm(lane *L, size_t text_bytes)
{
    L->armed = 0;
    if (!ticket_enabled() || !pinned_ready(L)) return;
    /* A riding ticket ends EVERY workgroup in a system-scope release (ticket_release: the L2 write-back of a grid
     * that is still writing its text); past a few hundred workgroups that costs more than the second launch it
     * saves (tools/sync_vs_async.py), so a long text gets k_ticket behind its kernel instead.                   */
    if (text_bytes > g_env.ticket_ride_max) return;
    L->armed = ticket_next(L);
    uaesk_ticket_arm((void *)ticket_word(L), L->d_status + 16, L->armed);
}

static void ticket_armed_launch_done(lane *L)
{
    if (uaesk_ticket_disarm()) L->armed = 0;                  /* nobody took it */
}

/* wait until everything queued on the lane's stream is done; n > 0: also bring n bytes (<= 64, a multiple of 4)
 * from device memory `dev` to `host`                                                                        */
static int lane_wait_fetch(lane *L, void *host, const void *dev, size_t n)
{
    hipStream_t st = (hipStream_t)L->stream;
    const uint32_t armed = L->armed;
    L->armed = 0;
    if (armed && n == 0) return ticket_wait(L, armed);        /* the call's kernel releases it itself */
    if (ticket_enabled() && n <= 64 && (n & 3u) == 0 && (((uintptr_t)dev) & 3u) == 0 && pinned_ready(L)) {
        void *data = (char *)L->pinx + TICKET_DATA_OFF;
        const uint32_t seq = ticket_next(L);
        int k = uaesk_ticket(L->stream, (void *)ticket_word(L), seq, dev, data, (unsigned)n);
        if (k == 0) {
            int rc = ticket_wait(L, seq);
            if (rc) return rc;
            if (n) memcpy(host, data, n);
            return 0;
        }
        (void)hipGetLastError();                              /* could not launch it: the plain way */
    }
    if (n) HIPCHK(hipMemcpyAsync(host, dev, n, hipMemcpyDefault, st));   /* dev may lie in the mapped pinned window */
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

static int lane_sync(lane *L)
{
    return lane_wait_fetch(L, NULL, NULL, 0);
}

/* 4 .. 16 bytes of result (status word, tag, MAC) from the lane's device slot to the host */
static int lane_fetch(lane *L, void *host, const void *dev, size_t n)
{
    return lane_wait_fetch(L, host, dev, n);
}

/* Where a synchronous call's kernels put their status word (0 / 0x1A): a word of the lane's pinned page when there
 * is one -- the host then reads it as soon as the stream has drained, no copy command, and a one-launch decryption can
 * carry the completion ticket itself -- else the lane's device slot.                                            */
static int *lane_status(lane *L)
{
    if (ticket_enabled() && pinned_ready(L)) return (int *)((char *)L->pinx + TICKET_OFF + 16);
    return L->d_status;
}

/* wait for the lane, then the status word its kernels wrote through `where` (= lane_status(L)) */
static int lane_read_status(lane *L, int *where, int *status)
{
    int rc;
    if (where == L->d_status) return lane_fetch(L, status, L->d_status, sizeof *status);
    if ((rc = lane_sync(L)) != 0) return rc;
    *status = *(volatile int *)where;
    return 0;
}

static int is_device_ptr(const void *p)
{
    hipPointerAttribute_t a;
    if (!p) return 0;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();                 /* plain host memory: clear the sticky error */
        return 0;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

/* A caller that hands the synchronous API DEVICE memory may have produced it with work still in
 * flight on the default stream (or streams that synchronise with it) -- the lane's stream is
 * non-blocking and would not wait for that by itself.                                        */
static __thread void *tls_producer_stream;      /* uaes_set_producer_stream(): NULL = the default stream */

static int wait_for_callers_device_work(void)
{
    HIPCHK(hipStreamSynchronize((hipStream_t)tls_producer_stream));
    return 0;
}

/* A caller whose device-resident input is produced on a stream of its own -- one created with hipStreamNonBlocking does
 * not synchronise with the default stream -- names it here (thread-local): every later synchronous call of this thread
 * that is handed device memory waits for THAT stream before it reads.  NULL = the default stream again.           */
int uaes_set_producer_stream(void *stream)
{
    tls_producer_stream = stream;
    return 0;
}

/* ---- long HOST texts over several GPUs without a change in the caller (UAES_DEVICES / uaes_set_devices) ----------
 * The reference's callers pass host pointers (micro_aes.h:173-181, :239-249, :256-266, :294-308) and one GPU's PCIe
 * link carries 25-33 GiB/s of such a text.  With a device list configured, the synchronous
 * ECB / CTR / XTS-sector / GCM calls hand a host text of at least min_bytes to the uaes_mgpu_* split, every device
 * staging its slice over its own link; results are bit-identical (the slices carry their counter / sector offsets and
 * GCM's shares are XORed on the host).  Off by default.  The workers of uaes_mgpu_* call the same entry points for
 * their slices: they are marked so that a slice is never split again.                                             */
static struct {
    int n, devs[MAX_DEVICES];
    size_t min_bytes;
    pthread_mutex_t mu;
} g_auto = { 0, { 0 }, (size_t)64 << 20, PTHREAD_MUTEX_INITIALIZER };
static __thread int tls_is_mgpu_worker;

static int set_devices(int ndev, const int *devices, size_t min_bytes)
{
    int i, avail = 0;
    if (ndev < -1 || ndev > MAX_DEVICES) return fail(UAES_E_ARG, "ndev must be -1 (all visible), 0 (off) or 1..%d", MAX_DEVICES);
    if (ndev != 0 && (hipGetDeviceCount(&avail) != hipSuccess || avail <= 0))
        return fail(UAES_E_HIP, "no usable HIP device; this library has no CPU path");
    if (ndev == -1) ndev = avail > MAX_DEVICES ? MAX_DEVICES : avail, devices = NULL;
    for (i = 0; i < ndev; ++i) {
        const int d = devices ? devices[i] : i;
        if (d < 0 || d >= avail || d >= MAX_DEVICES) return fail(UAES_E_ARG, "device %d is not one of the %d visible", d, avail);
    }
    pthread_mutex_lock(&g_auto.mu);
    g_auto.n = ndev;
    for (i = 0; i < ndev; ++i) g_auto.devs[i] = devices ? devices[i] : i;
    if (min_bytes) g_auto.min_bytes = min_bytes;
    pthread_mutex_unlock(&g_auto.mu);
    return 0;
}

int uaes_set_devices(int ndev, const int *devices, size_t min_bytes)
{
    env_ready();                                   /* (a later first call must not overwrite this with the environment) */
    return set_devices(ndev, devices, min_bytes);
}

static void auto_devices_from_env(void)          /* once, from env_init() */
{
    const char *e = getenv("UAES_DEVICES"), *m = getenv("UAES_DEVICES_MIN_MIB");
    int devs[MAX_DEVICES], n = 0;
    if (m && *m) { long v = strtol(m, NULL, 10); if (v >= 0) g_auto.min_bytes = v ? (size_t)v << 20 : 1; }
    if (!e || !*e) return;
    if (strcmp(e, "all") == 0) {
        if (set_devices(-1, NULL, 0) != 0) fprintf(stderr, "uaes-hip: UAES_DEVICES=all ignored: %s\n", uaes_last_error());
        return;
    }
    while (*e && n < MAX_DEVICES) {
        char *end = NULL;
        long v = strtol(e, &end, 10);
        if (end == e) break;
        devs[n++] = (int)v;
        e = end;
        while (*e == ',' || *e == ' ') ++e;
    }
    if (*e || n == 0 || set_devices(n, devs, 0) != 0)
        fprintf(stderr, "uaes-hip: UAES_DEVICES ignored (a comma-separated list of visible device ordinals, or \"all\")\n");
}

/* ---- the engine's own HOST data path (uaes_host.c): OFF unless the deployer switches it on --------------------------
 * By default every call runs on the GPU and fails loudly without one.  Three independent switches, process-wide:
 *   max_bytes  host-pointer calls of at most this many bytes run on the host (0 = never): below ~1 KiB (GCM ~200 B) a
 *              kernel launch costs more than the cipher (profiles/r04_break_even.md);
 *   chains     ONE serial chain given host pointers -- CBC / CFB encryption, OFB, CMAC, CCM -- runs on the host whatever
 *              its length: a chain is a latency-bound single wave on the GPU (36 MiB/s);
 *   fallback   with NO usable HIP device the modes this path implements run on the host instead of failing
 *              (a `void` function of the reference's API cannot report an error).
 * Environment, read once: UAES_HOST_MAX (bytes), UAES_HOST_CHAINS=1, UAES_HOST_FALLBACK=1.  Device pointers always go to
 * the GPU.  The batch / record / key-context / stream / mgpu / *_dev calls have no host path.                      */
static struct { size_t max_bytes, gcm_max_bytes; int chains, fallback, no_device; } g_host = { 0, 0, 0, 0, -1 };

int uaes_set_host_policy(size_t max_bytes, int chains, int fallback)
{
    env_ready();                                   /* (so that a later first call does not overwrite this with the environment) */
    __atomic_store_n(&g_host.max_bytes, max_bytes, __ATOMIC_RELEASE);
    __atomic_store_n(&g_host.chains, chains != 0, __ATOMIC_RELEASE);
    __atomic_store_n(&g_host.fallback, fallback != 0, __ATOMIC_RELEASE);
    return 0;
}

int uaes_get_host_policy(size_t *max_bytes, int *chains, int *fallback)
{
    env_ready();
    if (max_bytes) *max_bytes = __atomic_load_n(&g_host.max_bytes, __ATOMIC_ACQUIRE);
    if (chains) *chains = __atomic_load_n(&g_host.chains, __ATOMIC_ACQUIRE);
    if (fallback) *fallback = __atomic_load_n(&g_host.fallback, __ATOMIC_ACQUIRE);
    return 0;
}

static void host_policy_from_env(void)             /* once, from env_init() */
{
    const char *m = getenv("UAES_HOST_MAX"), *p = getenv("UAES_HOST_POLICY");
    /* UAES_HOST_POLICY=recommended: the measured crossover of this host class (profiles/r05_host_policy.md: the host path
     * is the faster one up to 4 KiB, GCM 2 KiB), single chains on the host, and a GPU-less box served instead of refused;
     * the individual variables refine it */
    if (p && strcmp(p, "recommended") == 0) { g_host.max_bytes = 4096; g_host.gcm_max_bytes = 2048; g_host.chains = 1; g_host.fallback = 1; }
    if (m && *m) { long long v = strtoll(m, NULL, 10); if (v >= 0) g_host.max_bytes = (size_t)v; }
    g_host.chains = env_int("UAES_HOST_CHAINS", g_host.chains, 0, 1);
    g_host.fallback = env_int("UAES_HOST_FALLBACK", g_host.fallback, 0, 1);
}

/* leaving through the host path: the schedule on the caller's stack is wiped (the reference BURNs its RoundKey after
 * every call, micro_aes.c:360) and a non-zero code gets its text in uaes_last_error() like the device path's */
static void burn(void *p, size_t n)
{
    volatile unsigned char *v = (volatile unsigned char *)p;
    while (n--) *v++ = 0;
}
static int host_result(int rc)
{
    if (rc == UAES_E_AUTHENTICATION) return fail(rc, "authentication failed (host path)");
    if (rc == UAES_E_DECRYPTION) return fail(rc, "ciphertext length is no multiple of the block size (host path)");
    if (rc == UAES_E_DATALENGTH) return fail(rc, "data too short (host path)");
    if (rc != 0) return fail(rc, "host path failed (%d)", rc);
    return 0;
}
#define HOST_RET(ksv, rc) do { const int hr_ = (rc); burn(&(ksv), sizeof (ksv)); return host_result(hr_); } while (0)

/* does this call run on the host path?  chain != 0: one serial chain; gcm != 0: GCM's own, lower crossover applies */
static int host_take_mode(const void *in, const void *out, size_t len, int chain, int gcm);
static int host_take(const void *in, const void *out, size_t len, int chain) { return host_take_mode(in, out, len, chain, 0); }
static int host_take_mode(const void *in, const void *out, size_t len, int chain, int gcm)
{
    size_t mx = __atomic_load_n(&g_host.max_bytes, __ATOMIC_ACQUIRE);
    const int ch = __atomic_load_n(&g_host.chains, __ATOMIC_ACQUIRE), fb = __atomic_load_n(&g_host.fallback, __ATOMIC_ACQUIRE);
    if (!mx && !ch && !fb) {
        env_ready();
        if (!g_host.max_bytes && !g_host.chains && !g_host.fallback) return 0;      /* the default: GPU, always */
        return host_take_mode(in, out, len, chain, gcm);
    }
    if (gcm && g_host.gcm_max_bytes && g_host.gcm_max_bytes < mx) mx = g_host.gcm_max_bytes;
    if (fb) {
        /* probed once -- and again after any HIP failure of this process: a GPU that goes away after the first call
         * must not keep the documented fallback from engaging */
        if (__atomic_exchange_n(&g_device_suspect, 0, __ATOMIC_ACQ_REL)) __atomic_store_n(&g_host.no_device, -1, __ATOMIC_RELEASE);
        if (g_host.no_device < 0) {
            int n = 0;
            const int none = hipGetDeviceCount(&n) != hipSuccess || n <= 0;
            (void)hipGetLastError();
            __atomic_store_n(&g_host.no_device, none, __ATOMIC_RELEASE);
        }
        if (g_host.no_device) return 1;
    }
    if (!(chain ? (ch || (mx && len <= mx)) : (mx && len <= mx))) return 0;
    return !is_device_ptr(in) && !is_device_ptr(out);
}

static uaesh_key host_key(const keysched *ks)
{
    uaesh_key k;
    k.ek = ks->ek.w; k.dk = ks->dk.w; k.nr = ks->nr;
    return k;
}

/* > 1: split this call over devs[0..n); 0: run it on the current device as always */
static int auto_devices(const void *in, const void *out, size_t len, int *devs)
{
    int n;
    if (tls_is_mgpu_worker) return 0;
    env_ready();
    if (g_auto.n < 2 || len < g_auto.min_bytes) return 0;
    if (is_device_ptr(in) || is_device_ptr(out)) return 0;
    pthread_mutex_lock(&g_auto.mu);
    n = g_auto.n;
    memcpy(devs, g_auto.devs, sizeof g_auto.devs);
    pthread_mutex_unlock(&g_auto.mu);
    return n < 2 ? 0 : n;
}

/* Resolve (in, out) to device pointers, staging whatever is host memory or
 * misaligned.  in_len bytes are copied in; the caller copies out_len back
 * with finish_io().                                                          */
typedef struct {
    const void *din;
    void       *dout;
    void       *user_out;
    size_t      out_len;
    int         copy_back;
    int         out_is_host;
    int         drained;            /* the caller has just waited for the lane (status fetch) and queued nothing since */
    lane       *L;
} io_plan;

/* Short host texts travel through pinned bounce buffers with asynchronous copies on the
 * lane's stream, so a call synchronises once instead of three times (pageable hipMemcpy
 * in, kernel, pageable hipMemcpy out): ~45 -> ~28 us for a 4 KiB call.  Shorter ones still
 * (zero_copy_max()) are not copied at all: the pinned buffers are mapped into the GPU's address
 * space, so the kernel reads the text from pin[0] and writes the result to pin[1] across the
 * link itself -- one submission per call instead of three (copy, kernel, copy).          */
static int env_int(const char *name, int dflt, int lo, int hi);

static size_t pin_bytes(void)
{
    env_ready();
    return g_env.pin_bytes;
}
#define PIN_BYTES pin_bytes()

static size_t zero_copy_max(void)
{
    env_ready();
    return g_env.zero_copy_max;
}

/* The ticket word, the fetched result bytes and the zero-copy windows are written by kernels and read by the host
 * after it has seen a flag change, with no runtime call in between: that needs fine-grained, coherent, GPU-mapped
 * host memory.  hipHostMallocDefault gives that only as long as nobody sets HIP_HOST_COHERENT=0, so it is asked for
 * by name; a runtime that refuses the flags gets the default request (and its default behaviour) instead.       */
static hipError_t pinned_alloc(void **p, size_t bytes)
{
    hipError_t e = hipHostMalloc(p, bytes, hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    }
    return e;
}

static int pinned_ready(lane *L)
{
    int i;
    for (i = 0; i < 2; ++i)
        if (!L->pin[i] && pinned_alloc(&L->pin[i], PIN_BYTES + 64) != hipSuccess) {
            (void)hipGetLastError();
            L->pin[i] = NULL;
            return 0;                             /* no pinned memory: the pageable path still works */
        }
    if (!L->pinx) {
        if (pinned_alloc(&L->pinx, 4096) != hipSuccess) {
            (void)hipGetLastError();
            L->pinx = NULL;
            return 0;
        }
        memset(L->pinx, 0, 4096);                 /* the ticket word must not hold a stale sequence number */
    }
    return 1;
}

static int plan_io(lane *L, const void *in, size_t in_len, void *out, size_t out_cap, io_plan *io)
{
    const int in_dev = in_len ? is_device_ptr(in) : 0, out_dev = out_cap ? is_device_ptr(out) : 0;
    const int in_ok = in_len == 0 || (in_dev && (((uintptr_t)in) & 15u) == 0);
    const int out_ok = out_cap == 0 || (out_dev && (((uintptr_t)out) & 15u) == 0);
    hipStream_t st = (hipStream_t)L->stream;
    io->user_out = out;
    io->drained = 0;
    io->copy_back = !out_ok;
    io->out_is_host = !out_dev;
    io->din = in;
    io->dout = out;
    io->L = L;
    if (in_dev || out_dev) { int rc = wait_for_callers_device_work(); if (rc) return rc; }
    /* every call ends with the lane's stream drained (finish_io / lane_fetch, and the error paths
     * below the API boundary go through lane_abandon), so the bounce buffers are free here      */
    if (!in_dev && !out_dev && in_len <= zero_copy_max() && out_cap <= zero_copy_max() && pinned_ready(L)) {
        if (in_len) { memcpy(L->pin[0], in, in_len); io->din = L->pin[0]; }
        if (out_cap) io->dout = L->pin[1];        /* finish_io hands it over from there */
        return 0;
    }
    if (!in_ok) {
        const size_t need = (in_len > out_cap ? in_len : out_cap) + 64;
        if (grow_on(st, &L->stage[0], &L->stage_cap[0], need)) return UAES_E_HIP;
        if (in_len <= PIN_BYTES && !in_dev && pinned_ready(L)) {
            memcpy(L->pin[0], in, in_len);
            HIPCHK(hipMemcpyAsync(L->stage[0], L->pin[0], in_len, hipMemcpyHostToDevice, st));
        } else {
            HIPCHK(hipMemcpyAsync(L->stage[0], in, in_len, hipMemcpyDefault, st));
        }
        io->din = L->stage[0];
        if (!out_ok) io->dout = L->stage[0];      /* run in place in the staging buffer */
    } else if (!out_ok) {
        if (grow_on(st, &L->stage[1], &L->stage_cap[1], out_cap + 64)) return UAES_E_HIP;
        io->dout = L->stage[1];
    }
    return 0;
}

static int finish_io(io_plan *io, size_t out_len)
{
    lane *L = io->L;
    hipStream_t st = (hipStream_t)L->stream;
    int rc;
    if (io->dout && io->dout == L->pin[1]) {      /* the kernel wrote the mapped pinned buffer itself */
        if (!io->drained && (rc = lane_sync(L)) != 0) return rc;
        if (out_len) memcpy(io->user_out, L->pin[1], out_len);
        return 0;
    }
    if (io->copy_back && out_len && out_len <= PIN_BYTES && io->out_is_host && pinned_ready(L)) {
        L->armed = 0;                             /* a copy follows the kernel: the stream is drained the plain way */
        HIPCHK(hipMemcpyAsync(L->pin[1], io->dout, out_len, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        memcpy(io->user_out, L->pin[1], out_len);
        return 0;
    }
    if (io->copy_back && out_len) {
        L->armed = 0;
        HIPCHK(hipMemcpyAsync(io->user_out, io->dout, out_len, hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    return io->drained ? 0 : lane_sync(L);
}

/* a call bails out with work possibly queued on the lane: nothing of it may still be running
 * (or reading the bounce buffers) when the next call of this thread starts                    */
static int lane_abandon(lane *L, int rc)
{
    if (L) L->armed = 0;
    (void)uaesk_ticket_disarm();
    if (L && L->stream) {
        (void)hipStreamSynchronize((hipStream_t)L->stream);
        if (L->scratch) (void)hipMemsetAsync(scratch_done_word(L->scratch, L->scratch_cap), 0, SCRATCH_TAIL, (hipStream_t)L->stream);
        repair_done_word(L->stream);                  /* a key context's word, if that is what this call armed */
    }
    return rc;
}

/* ------------------------------------------------------------------------ */
/* long host texts: slices in flight on several streams                        */
/* ------------------------------------------------------------------------ */
/* The reference's callers pass HOST buffers.  One big hipMemcpy in, the kernel, one big
 * hipMemcpy out use the PCIe link in one direction at a time (25 GiB/s for a 1 GiB CTR call
 * of which the kernel is 0.65 ms).  For the modes whose blocks are independent (ECB, CTR, XTS
 * data units) a long text is cut into slices and PIPE_WORKERS host threads each take the
 * next slice: copy in, kernel, copy out on the worker's own stream and device slice, so the
 * two DMA directions and the staging copies of different slices overlap: 33 GiB/s with four
 * workers (profiles/HISTORY.md; 1.29x -- the link gives ~36 GB/s each way when both
 * directions run; staging through our own pinned buffers measured slower, 26-29 GiB/s, the
 * runtime's pageable path copies faster than memcpy() from worker threads does).  The workers
 * touch only c->pipe[w] and read-only context data; one pipelined call at a time per device
 * (the link is the bottleneck, a second call would only queue behind it).                  */
#define PIPE_MIN      ((size_t)32 << 20)          /* shorter texts: the plain path            */
#define PIPE_MAXW     16

typedef int (*pipe_launch_fn)(void *arg, int worker, void *stream, const void *d_in, void *d_out, size_t off, size_t len);

typedef struct {
    context       *c;
    int            device, worker;
    const char    *in;
    char          *out;
    size_t         total, slice, out_extra;       /* out_extra: bytes the LAST slice writes beyond its input size */
    size_t        *next;                          /* shared: offset of the next slice to take  */
    pthread_mutex_t *next_mu;
    pipe_launch_fn fn;
    void          *arg;
    int            rc;
    char           err[256];
} pipe_job;

static int env_int(const char *name, int dflt, int lo, int hi)
{
    const char *e = getenv(name);
    long v = dflt;
    if (e && *e) {
        char *end = NULL;
        v = strtol(e, &end, 10);
        if (end == e) v = dflt;                   /* not a number: the default */
    }
    if (v < lo) v = lo;
    if (v > hi) v = hi;
    return (int)v;
}

static void env_init(void)
{
    g_env.ticket = env_int("UAES_TICKET", 1, 0, 1);
    g_env.ticket_ride_max = (size_t)env_int("UAES_TICKET_RIDE_MAX_KIB", TICKET_RIDE_MAX_KIB, 0, 1 << 30) << 10;
    g_env.gcm_key_cache = env_int("UAES_GCM_KEY_CACHE", 1, 0, 1);
    g_env.pin_bytes = (size_t)env_int("UAES_PIN_KIB", 1024, 16, 65536) << 10;
    g_env.zero_copy_max = (size_t)env_int("UAES_ZEROCOPY_MAX_KIB", 1024, 0, (int)(g_env.pin_bytes >> 10)) << 10;
    g_env.pipe_workers = env_int("UAES_PIPE_WORKERS", 4, 1, PIPE_MAXW);
    g_env.pipe_slice = (size_t)env_int("UAES_PIPE_SLICE_MIB", 16, 1, 1024) << 20;
    auto_devices_from_env();
    host_policy_from_env();
}

static int pipe_workers(void)
{
    env_ready();
    return g_env.pipe_workers;
}

static size_t pipe_slice_bytes(void)
{
    env_ready();
    return g_env.pipe_slice;
}

#define PFAIL(j, ...) do { (j)->rc = UAES_E_HIP; snprintf((j)->err, sizeof (j)->err, __VA_ARGS__); return NULL; } while (0)

static void *pipe_worker(void *p)
{
    pipe_job *j = (pipe_job *)p;
    context *c = j->c;
    hipError_t e = hipSetDevice(j->device);
    if (e != hipSuccess) PFAIL(j, "hipSetDevice: %s", hipGetErrorString(e));
    hipStream_t st = (hipStream_t)c->pipe[j->worker].stream;
    char *d = (char *)c->pipe[j->worker].dbuf;
    for (;;) {
        size_t off, len, olen;
        pthread_mutex_lock(j->next_mu);
        off = *j->next;
        len = j->total - off < j->slice ? j->total - off : j->slice;
        *j->next = off + len;
        pthread_mutex_unlock(j->next_mu);
        if (len == 0) return NULL;
        olen = len + (off + len == j->total ? j->out_extra : 0);
        e = hipMemcpyAsync(d, j->in + off, len, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) PFAIL(j, "slice copy in: %s", hipGetErrorString(e));
        int k = j->fn(j->arg, j->worker, st, d, d, off, len);
        if (k > 0) PFAIL(j, "slice launch: %s", hipGetErrorString((hipError_t)k));
        if (k < 0) PFAIL(j, "slice at offset %zu: %s", off, uaes_last_error());   /* this thread's message */
        e = hipMemcpyAsync(j->out + off, d, olen, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) PFAIL(j, "slice copy out: %s", hipGetErrorString(e));
    }
}

/* returns 1 if the call qualifies (both buffers plain host memory, long enough), and then *rc is its result */
static int run_pipelined(context *c, const void *in, void *out, size_t total, size_t unit, size_t out_extra,
                         pipe_launch_fn fn, void *arg, int *rc)
{
    pipe_job jobs[PIPE_MAXW];
    pthread_t th[PIPE_MAXW];
    pthread_mutex_t next_mu = PTHREAD_MUTEX_INITIALIZER;
    size_t next = 0, slice = pipe_slice_bytes();
    int w, started = 0, nw = pipe_workers(), dev = 0;
    if (total < PIPE_MIN || nw < 2 || is_device_ptr(in) || is_device_ptr(out)) return 0;
    if (unit > slice) return 0;
    slice -= slice % unit;
    if (slice * 2 > total) return 0;
    if ((size_t)nw > (total + slice - 1) / slice) nw = (int)((total + slice - 1) / slice);
    *rc = 0;
    if (hipGetDevice(&dev) != hipSuccess) { *rc = fail(UAES_E_HIP, "hipGetDevice failed"); return 1; }
    pthread_mutex_lock(&c->mu);
    while (c->pipe_busy) pthread_cond_wait(&c->cv, &c->mu);
    for (w = 0; w < nw && *rc == 0; ++w) {
        if (!c->pipe[w].stream && hipStreamCreateWithFlags((hipStream_t *)&c->pipe[w].stream, hipStreamNonBlocking) != hipSuccess)
            *rc = fail(UAES_E_HIP, "pipeline stream creation failed");
        if (*rc == 0 && !c->pipe[w].dbuf && hipMalloc(&c->pipe[w].dbuf, pipe_slice_bytes() + 64) != hipSuccess)
            *rc = fail(UAES_E_HIP, "pipeline slice allocation failed");
    }
    if (*rc) { pthread_mutex_unlock(&c->mu); return 1; }
    c->pipe_busy = 1;                             /* pipe[] is ours until the workers have joined */
    pthread_mutex_unlock(&c->mu);
    memset(jobs, 0, sizeof jobs);
    for (w = 0; w < nw; ++w) {
        jobs[w].c = c; jobs[w].device = dev; jobs[w].worker = w;
        jobs[w].in = (const char *)in; jobs[w].out = (char *)out; jobs[w].total = total; jobs[w].slice = slice;
        jobs[w].out_extra = out_extra; jobs[w].next = &next; jobs[w].next_mu = &next_mu; jobs[w].fn = fn; jobs[w].arg = arg;
        if (pthread_create(&th[w], NULL, pipe_worker, &jobs[w]) != 0) { *rc = fail(UAES_E_HIP, "pthread_create failed"); break; }
        ++started;
    }
    for (w = 0; w < started; ++w) pthread_join(th[w], NULL);
    pthread_mutex_lock(&c->mu);
    c->pipe_busy = 0;
    pthread_cond_broadcast(&c->cv);
    pthread_mutex_unlock(&c->mu);
    for (w = 0; w < started && *rc == 0; ++w)
        if (jobs[w].rc) *rc = fail(jobs[w].rc, "%s", jobs[w].err);
    return 1;
}

/* a decrypt-then-verify mode found a bad tag: hand the text over as the reference's default
 * build does, or (uaes_set_wipe_on_auth_failure) hand over zeros instead               */
static int finish_io_unauthenticated(io_plan *io, size_t out_len)
{
    lane *L = io->L;
    if (!wipe_on_auth_failure()) return finish_io(io, out_len);
    if (out_len && !io->out_is_host)
        HIPCHK(hipMemsetAsync(io->user_out, 0, out_len, (hipStream_t)L->stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)L->stream));
    if (out_len && io->out_is_host) memset(io->user_out, 0, out_len);
    return 0;
}

/* the *_dev entry points hand their pointers straight to the kernels (uint4 accesses) */
static int dev_ptrs_ok(const void *in, const void *out, size_t len)
{
    if (len && (!in || !out)) return fail(UAES_E_ARG, "NULL device pointer");
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 15u)
        return fail(UAES_E_ARG, "device pointers of the *_dev API must be 16-byte aligned");
    return 0;
}

/* the synchronous entry points run between enter() and DONE(): the latter drains the lane when the
 * call did not end in finish_io / lane_fetch (an error in the middle)                              */
static int lane_leave(lane *L, int rc)
{
    if (rc < 0) rc = lane_abandon(L, rc);
    tls_armed_word = NULL;                           /* the word may belong to a key context the caller frees next */
    return rc;
}
#define DONE(L, rc) return lane_leave((L), (rc))

/* ------------------------------------------------------------------------ */
/* housekeeping API                                                           */
/* ------------------------------------------------------------------------ */
int uaes_stream_release(void *stream)
{
    context *c;
    int rc, i;
    if ((rc = get_context(&c)) != 0) return rc;
    pthread_mutex_lock(&c->mu);
    rc = 0;
    for (i = 0; i < SCRATCH_SLOTS; ++i) {
        if (!c->slot[i].used || c->slot[i].stream != stream) continue;
        while (c->slot[i].pins > 0) pthread_cond_wait(&c->cv, &c->mu);
        if (c->slot[i].buf) {
            if (hipDeviceSynchronize() != hipSuccess || hipFree(c->slot[i].buf) != hipSuccess)
                rc = fail(UAES_E_HIP, "uaes_stream_release: freeing the scratch failed");
        }
        memset(&c->slot[i], 0, sizeof c->slot[i]);
        break;
    }
    pthread_mutex_unlock(&c->mu);
    return rc;
}

int uaes_init(void)
{
    context *c;
    return get_context(&c);
}

static void gather_teardown(void);                 /* the cached RCCL communicators and streams of uaes_mgpu_ctr_encrypt_gather */

int uaes_shutdown(void)
{
    int d, i, prev = -1, rc = 0;
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    gather_teardown();
    pthread_mutex_lock(&g_init_mu);
    for (d = 0; d < MAX_DEVICES; ++d) {
        context *c = &g_ctx[d];
        lane *L;
        if (!c->ready) continue;
        if (hipSetDevice(d) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            rc = fail(UAES_E_HIP, "uaes_shutdown: device %d is not usable", d);
            continue;
        }
        pthread_mutex_lock(&c->mu);
        for (L = c->lanes; L; L = L->next) lane_free_resources(L);   /* the structs stay with their threads */
        for (i = 0; i < PIPE_MAXW; ++i) {
            if (c->pipe[i].dbuf) (void)hipFree(c->pipe[i].dbuf);
            if (c->pipe[i].xscratch) {
                (void)hipMemset(c->pipe[i].xscratch, 0, c->pipe[i].xscratch_cap);   /* may hold GHASH tables (the GCM pipeline) */
                (void)hipFree(c->pipe[i].xscratch);
            }
            if (c->pipe[i].stream) (void)hipStreamDestroy((hipStream_t)c->pipe[i].stream);
            memset(&c->pipe[i], 0, sizeof c->pipe[i]);
        }
        for (i = 0; i < c->nspool; ++i) (void)hipFree(c->spool[i]);   /* (wiped when they were put there) */
        c->nspool = 0;
        for (i = 0; i < SCRATCH_SLOTS; ++i) {
            if (c->slot[i].buf) {
                (void)hipMemset(c->slot[i].buf, 0, c->slot[i].cap);  /* GHASH tables are key material */
                (void)hipFree(c->slot[i].buf);
            }
            memset(&c->slot[i], 0, sizeof c->slot[i]);
        }
        if (c->d_tables) (void)hipFree(c->d_tables);
        c->d_tables = NULL;
        memset(&c->tb, 0, sizeof c->tb);
        c->ready = 0;                             /* the next call builds the context again */
        pthread_mutex_unlock(&c->mu);
        (void)hipGetLastError();
    }
    pthread_mutex_unlock(&g_init_mu);
    if (prev >= 0) (void)hipSetDevice(prev);
    return rc;
}

/* enqueue the shader-clock probe (uaes_device.h) on `stream`: d_out16 receives { shader cycles, 100 MHz ticks } */
int uaes_clock_probe_dev(void *d_out16, unsigned spin_us, void *stream)
{
    context *c;
    int rc;
    if (!d_out16) return fail(UAES_E_ARG, "NULL pointer");
    if (spin_us > 1000000u) spin_us = 1000000u;                /* a wave that spins: never longer than a second */
    if ((rc = get_context(&c)) != 0) return rc;
    KCHK(uaesk_clock_probe(stream, d_out16, 100ull * spin_us));
    return 0;
}

int uaes_selftest(void)
{
    context *c;
    lane *L;
    keysched ks;
    uint8_t key[16];
    unsigned result = 0;
    int i, rc;
    if ((rc = enter(&c, &L)) != 0) return rc;
    for (i = 0; i < 16; ++i) key[i] = (uint8_t)i;
    if ((rc = expand_key(&ks, key, 128)) != 0) return rc;
    do {
        unsigned *d = (unsigned *)L->d_status;
        if (hipMemsetAsync(d, 0, 4, (hipStream_t)L->stream) != hipSuccess) { rc = fail(UAES_E_HIP, "hipMemset failed"); break; }
        int k = uaesk_selftest(L->stream, &c->tb, &ks.ek, &ks.dk, d);
        if (k) { rc = fail(UAES_E_HIP, "selftest launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if ((rc = lane_fetch(L, &result, d, 4)) != 0) break;
        rc = (int)result;
    } while (0);
    DONE(L, rc);
}

/* ------------------------------------------------------------------------ */
/* ECB                                                                        */
/* ------------------------------------------------------------------------ */
typedef struct { context *c; keysched *ks; int decrypt, padding; size_t total; } ecb_pipe_arg;

static int ecb_pipe_launch(void *arg, int worker, void *stream, const void *d_in, void *d_out, size_t off, size_t len)
{
    ecb_pipe_arg *a = (ecb_pipe_arg *)arg;
    (void)worker;
    const int last = off + len == a->total;
    return uaesk_ecb(stream, &a->c->tb, a->ks->nr, a->decrypt ? &a->ks->dk : &a->ks->ek, a->decrypt, d_in, d_out,
                     len / 16, (a->decrypt || !last) ? 0 : (unsigned)(len % 16), (last && !a->decrypt) ? (unsigned)a->padding : 0);
}

static int ecb_common(int keybits, const uint8_t *key, int decrypt, int padding,
                      const void *in, size_t len, void *out)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    int rc;
    const size_t rem = len % 16, nfull = len / 16;
    const size_t out_len = decrypt ? len : (padding ? (len / 16 + 1) * 16 : (len + 15) / 16 * 16);
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (padding < 0 || padding > 2) return fail(UAES_E_ARG, "padding must be 0 (zeros), 1 (PKCS#7) or 2 (ISO/IEC 7816-4)");
    if (out_len == 0) return 0;
    if ((len && !in) || !out) return fail(UAES_E_ARG, "NULL data pointer");
    if (host_take(in, out, len, 0)) {
        const uaesh_key hk = host_key(&ks);
        if (!decrypt) { uaesh_ecb_encrypt(&hk, padding, (const uint8_t *)in, len, (uint8_t *)out); HOST_RET(ks, 0); }
        uaesh_ecb_decrypt(&hk, (const uint8_t *)in, len, (uint8_t *)out);
        HOST_RET(ks, rem ? UAES_E_DECRYPTION : 0);
    }
    {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(in, out, len, devs);
        if (nd) return decrypt ? uaes_mgpu_ecb_decrypt(nd, devs, keybits, key, in, len, out)
                               : uaes_mgpu_ecb_encrypt(nd, devs, keybits, key, padding, in, len, out);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        ecb_pipe_arg pa;
        pa.c = c; pa.ks = &ks; pa.decrypt = decrypt; pa.padding = padding; pa.total = len;
        if (!(decrypt && rem) && run_pipelined(c, in, out, len, 16, out_len - len, ecb_pipe_launch, &pa, &rc)) return rc;
        if ((rc = plan_io(L, in, len, out, out_len, &io)) != 0) break;
        if (decrypt && rem && io.dout != io.din) {
            /* ragged decrypt: the reference copies the tail through (:664) */
            if (hipMemcpyAsync((char *)io.dout + nfull * 16, (const char *)io.din + nfull * 16, rem,
                               hipMemcpyDeviceToDevice, (hipStream_t)L->stream) != hipSuccess) {
                rc = fail(UAES_E_HIP, "tail copy failed");
                break;
            }
        }
        ticket_arm(L, len);
        int k = uaesk_ecb(L->stream, &c->tb, ks.nr, decrypt ? &ks.dk : &ks.ek, decrypt,
                          io.din, io.dout, nfull, decrypt ? 0 : (unsigned)rem, decrypt ? 0 : (unsigned)padding);
        ticket_armed_launch_done(L);
        if (k) { rc = fail(UAES_E_HIP, "ecb launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if ((rc = finish_io(&io, out_len)) != 0) break;
        rc = (decrypt && rem) ? UAES_E_DECRYPTION : 0;           /* :679 */
    } while (0);
    DONE(L, rc);
}

int uaes_ecb_encrypt(int keybits, const uint8_t *key, const void *pntxt, size_t ptextLen, void *crtxt)
{
    return ecb_common(keybits, key, 0, 0, pntxt, ptextLen, crtxt);
}

int uaes_ecb_encrypt_padded(int keybits, const uint8_t *key, int padding,
                            const void *pntxt, size_t ptextLen, void *crtxt)
{
    return ecb_common(keybits, key, 0, padding, pntxt, ptextLen, crtxt);
}

int uaes_ecb_decrypt(int keybits, const uint8_t *key, const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return ecb_common(keybits, key, 1, 0, crtxt, crtxtLen, pntxt);
}

int uaes_ecb_dev(int keybits, const uint8_t *key, int decrypt,
                 const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    keysched ks;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    if (decrypt && len % 16) return fail(UAES_E_ARG, "uaes_ecb_dev: ragged decrypt length");
    KCHK(uaesk_ecb(stream, &c->tb, ks.nr, decrypt ? &ks.dk : &ks.ek, decrypt, d_in, d_out,
                   len / 16, (unsigned)(len % 16), 0));
    return 0;
}

/* ------------------------------------------------------------------------ */
/* CTR                                                                        */
/* ------------------------------------------------------------------------ */
static void make_ctr(uaesk_ctr *c, const uint8_t ctr0[16], uint64_t block_offset)
{
    uint64_t v = 0;
    int i;
    memset(c, 0, sizeof *c);
    memcpy(&c->w0, ctr0, 4);
    memcpy(&c->w1, ctr0 + 4, 4);
    c->b8 = ctr0[8];
    for (i = 9; i < 16; ++i) v = (v << 8) | ctr0[i];
    c->v0 = (v + block_offset) & 0x00FFFFFFFFFFFFFFull;         /* 56-bit, N2 */
}

int uaes_ctr_xcrypt_at_dev(int keybits, const uint8_t *key, const uint8_t ctr0[16],
                           uint64_t block_offset,
                           const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    keysched ks;
    uaesk_ctr ctr;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if (!ctr0) return fail(UAES_E_ARG, "NULL counter block");
    if ((rc = get_context(&c)) != 0) return rc;
    make_ctr(&ctr, ctr0, block_offset);
    KCHK(uaesk_ctr_xcrypt(stream, &c->tb, ks.nr, &ks.ek, &ctr, d_in, d_out, len, NULL));
    return 0;
}

typedef struct { context *c; keysched *ks; uaesk_ctr *ctr; } ctr_pipe_arg;

static int ctr_pipe_launch(void *arg, int worker, void *stream, const void *d_in, void *d_out, size_t off, size_t len)
{
    ctr_pipe_arg *a = (ctr_pipe_arg *)arg;
    (void)worker;
    uaesk_ctr sl = *a->ctr;
    sl.v0 = (a->ctr->v0 + off / 16) & 0x00FFFFFFFFFFFFFFull;     /* the slice's counter: the 56-bit add of incBlock */
    return uaesk_ctr_xcrypt(stream, &a->c->tb, a->ks->nr, &a->ks->ek, &sl, d_in, d_out, len, NULL);
}

int uaes_ctr_xcrypt_at(int keybits, const uint8_t *key, const uint8_t ctr0[16],
                       uint64_t block_offset, const void *in, size_t len, void *out)
{
    context *c;
    lane *L;
    keysched ks;
    uaesk_ctr ctr;
    io_plan io;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!ctr0) return fail(UAES_E_ARG, "NULL counter block");
    if (len == 0) return 0;
    if (!in || !out) return fail(UAES_E_ARG, "NULL data pointer");
    if (host_take(in, out, len, 0)) {
        const uaesh_key hk = host_key(&ks);
        uaesh_ctr(&hk, ctr0, block_offset, (const uint8_t *)in, len, (uint8_t *)out);
        HOST_RET(ks, 0);
    }
    {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(in, out, len, devs);
        if (nd) return uaes_mgpu_ctr_xcrypt_at(nd, devs, keybits, key, ctr0, block_offset, in, len, out);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    make_ctr(&ctr, ctr0, block_offset);
    do {
        ctr_pipe_arg pa;
        pa.c = c; pa.ks = &ks; pa.ctr = &ctr;
        if (run_pipelined(c, in, out, len, 16, 0, ctr_pipe_launch, &pa, &rc)) return rc;
        if ((rc = plan_io(L, in, len, out, len, &io)) != 0) break;
        ticket_arm(L, len);
        int k = uaesk_ctr_xcrypt(L->stream, &c->tb, ks.nr, &ks.ek, &ctr, io.din, io.dout, len, NULL);
        ticket_armed_launch_done(L);
        if (k) { rc = fail(UAES_E_HIP, "ctr launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, len);
    } while (0);
    DONE(L, rc);
}

/* ivLen / startValue = the reference's compile-time CTR_IV_LENGTH / CTR_START_VALUE (micro_aes.h:98-99): the counter
 * block is the IV's first ivLen bytes with zeros behind them, and the start value XORed in as a big-endian integer
 * that ends at byte 15 (micro_aes.c:968-971, xorBEint :410-415)                                                   */
int uaes_ctr_xcrypt_iv(int keybits, const uint8_t *key, const uint8_t *iv, size_t ivLen, uint64_t startValue,
                       const void *in, size_t len, void *out)
{
    uint8_t ctr0[16] = { 0 };
    int pos = 15;
    if (!iv && ivLen) return fail(UAES_E_ARG, "NULL iv");
    if (ivLen > 16) return fail(UAES_E_ARG, "CTR IV length %zu (at most 16)", ivLen);
    if (ivLen) memcpy(ctr0, iv, ivLen);
    do ctr0[pos--] ^= (uint8_t)startValue; while ((startValue >>= 8) != 0);
    return uaes_ctr_xcrypt_at(keybits, key, ctr0, 0, in, len, out);
}

int uaes_ctr_xcrypt(int keybits, const uint8_t *key, const uint8_t *iv,
                    const void *in, size_t len, void *out)
{
    if (!iv) return fail(UAES_E_ARG, "NULL iv");
    return uaes_ctr_xcrypt_iv(keybits, key, iv, 12, 1, in, len, out);      /* CTR_IV_LENGTH 12, CTR_START_VALUE 1 */
}

/* ------------------------------------------------------------------------ */
/* XTS                                                                        */
/* ------------------------------------------------------------------------ */
static int xts_keys(keysched *k1, keysched *k2, const uint8_t *keys, int keybits)
{
    int rc;
    if (!keys) return fail(UAES_E_ARG, "NULL key pair");
    if ((rc = expand_key(k1, keys, keybits)) != 0) return rc;
    return expand_key(k2, keys + keybits / 8, keybits);          /* :1026-1029 */
}

/* scratch == NULL: the *_dev path -- take (and pin) the slot of the caller's stream */
static int xts_run(context *c, void *stream, keysched *k1, keysched *k2, int encrypt,
                   const uint8_t *tweak16, uint64_t first_sector,
                   size_t sector_bytes, size_t nsectors, const void *din, void *dout, void *scratch)
{
    int slot = -1, k;
    if (!scratch) {
        pthread_mutex_lock(&c->mu);
        const int g = scratch_pin(c, stream, uaesk_xts_scratch_bytes(sector_bytes, nsectors), &scratch, &slot);
        pthread_mutex_unlock(&c->mu);
        if (g) return UAES_E_HIP;
    }
    k = uaesk_xts(stream, &c->tb, k1->nr, encrypt ? &k1->ek : &k1->dk, &k2->ek, !encrypt,
                  tweak16, first_sector, sector_bytes, nsectors, din, dout, scratch);
    if (slot >= 0) scratch_unpin(c, slot);
    if (k) return fail(UAES_E_HIP, "xts launch: %s", hipGetErrorString((hipError_t)k));
    return 0;
}

typedef struct { context *c; keysched *k1, *k2; int encrypt; uint64_t first_sector; size_t sector_bytes; } xts_pipe_arg;

/* a pipeline worker keeps its own chunk-tweak scratch next to its device slice: it never takes one of
 * the per-stream slots of the *_dev API (which it used to occupy for the life of the process)       */
static int xts_pipe_launch(void *arg, int worker, void *stream, const void *d_in, void *d_out, size_t off, size_t len)
{
    xts_pipe_arg *a = (xts_pipe_arg *)arg;
    context *c = a->c;
    const size_t ns = len / a->sector_bytes;
    if (grow_on(stream, &c->pipe[worker].xscratch, &c->pipe[worker].xscratch_cap,
                uaesk_xts_scratch_bytes(a->sector_bytes, ns)))
        return -1;
    return xts_run(c, stream, a->k1, a->k2, a->encrypt, NULL, a->first_sector + off / a->sector_bytes,
                   a->sector_bytes, ns, d_in, d_out, c->pipe[worker].xscratch) ? -1 : 0;
}

static int xts_common(int keybits, const uint8_t *keys, const uint8_t *tweak, int raw_tweak,
                      uint64_t first_sector, size_t sector_bytes, size_t nsectors,
                      const void *in, void *out, int encrypt)
{
    context *c;
    lane *L;
    keysched k1, k2;
    io_plan io;
    uint8_t zero[16] = { 0 };
    int rc;
    const size_t total = sector_bytes * nsectors;
    if ((rc = xts_keys(&k1, &k2, keys, keybits)) != 0) return rc;
    if (sector_bytes < 16) return UAES_E_DATALENGTH;             /* :1069, untouched */
    if (nsectors == 0) return 0;
    if (!in || !out) return fail(UAES_E_ARG, "NULL data pointer");
    if (host_take(in, out, total, 0)) {
        const uaesh_key h1 = host_key(&k1), h2 = host_key(&k2);
        if (raw_tweak) uaesh_xts_unit(&h1, &h2, encrypt, tweak ? tweak : zero, (const uint8_t *)in, sector_bytes, (uint8_t *)out);
        else uaesh_xts_sectors(&h1, &h2, encrypt, first_sector, sector_bytes, nsectors, (const uint8_t *)in, (uint8_t *)out);
        do { burn(&k2, sizeof k2); HOST_RET(k1, 0); } while (0);
    }
    if (!raw_tweak && nsectors > 1) {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(in, out, total, devs);
        if (nd) return uaes_mgpu_xts_sectors(nd, devs, keybits, keys, first_sector, sector_bytes, nsectors, in, out, encrypt);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        xts_pipe_arg pa;
        pa.c = c; pa.k1 = &k1; pa.k2 = &k2; pa.encrypt = encrypt; pa.first_sector = first_sector; pa.sector_bytes = sector_bytes;
        if (!raw_tweak && nsectors > 1 && run_pipelined(c, in, out, total, sector_bytes, 0, xts_pipe_launch, &pa, &rc)) return rc;
        if ((rc = lane_scratch(L, uaesk_xts_scratch_bytes(sector_bytes, nsectors), SCRATCH_OTHER)) != 0) break;
        if ((rc = plan_io(L, in, total, out, total, &io)) != 0) break;
        ticket_arm(L, total);
        rc = xts_run(c, L->stream, &k1, &k2, encrypt, raw_tweak ? (tweak ? tweak : zero) : NULL,
                     first_sector, sector_bytes, nsectors, io.din, io.dout, L->scratch);
        ticket_armed_launch_done(L);
        if (rc) break;
        rc = finish_io(&io, total);
    } while (0);
    DONE(L, rc);
}

int uaes_xts_encrypt(int keybits, const uint8_t *keys, const uint8_t *tweak,
                     const void *pntxt, size_t ptextLen, void *crtxt)
{
    return xts_common(keybits, keys, tweak, 1, 0, ptextLen, 1, pntxt, crtxt, 1);
}

int uaes_xts_decrypt(int keybits, const uint8_t *keys, const uint8_t *tweak,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return xts_common(keybits, keys, tweak, 1, 0, crtxtLen, 1, crtxt, pntxt, 0);
}

int uaes_xts_sectors(int keybits, const uint8_t *keys, uint64_t first_sector,
                     size_t sector_bytes, size_t nsectors, const void *in, void *out, int encrypt)
{
    return xts_common(keybits, keys, NULL, 0, first_sector, sector_bytes, nsectors, in, out, encrypt);
}

int uaes_xts_sectors_dev(int keybits, const uint8_t *keys, uint64_t first_sector,
                         size_t sector_bytes, size_t nsectors,
                         const void *d_in, void *d_out, int encrypt, void *stream)
{
    context *c;
    keysched k1, k2;
    int rc;
    if ((rc = xts_keys(&k1, &k2, keys, keybits)) != 0) return rc;
    if ((rc = dev_ptrs_ok(d_in, d_out, sector_bytes * nsectors)) != 0) return rc;
    if (sector_bytes < 16) return UAES_E_DATALENGTH;
    if ((rc = get_context(&c)) != 0) return rc;
    return xts_run(c, stream, &k1, &k2, encrypt, NULL, first_sector, sector_bytes, nsectors, d_in, d_out, NULL);
}

/* ------------------------------------------------------------------------ */
/* GCM                                                                        */
/* ------------------------------------------------------------------------ */
static int gcm_scratch(lane *L, int owner)       /* synchronous API: the thread's own scratch */
{
    return lane_scratch(L, uaesk_gcm_scratch_bytes(), owner);
}

/* 1: the tables of `key` are in the lane's scratch (this call may run as a call on a key context, uaesk_gcm_keyed),
 * 0: they are not (the one-shot path), < 0: error.  Call with the scratch allocated (gcm_scratch).  A call on a key
 * context is 2-4 us shorter than a one-shot call and the table set costs ~20 us once, so it is built when the EIGHTH
 * call in a row comes under one key (a sequence that stops there has lost those 20 us, a longer one gains 10-15 %
 * per call); UAES_GCM_KEY_CACHE=0 switches the cache off.                                                     */
#define GK_BUILD_AT 8
#define GK_TABLES   255
static int lane_gcm_keyed(lane *L, const keysched *ks, const uint8_t *key, int keybits)
{
    const size_t kb = (size_t)keybits / 8;
    if (!g_env.gcm_key_cache || !L->c->tb.frob) return 0;
    if (L->gk_state && L->gk_bits == keybits && memcmp(L->gk, key, kb) == 0) {
        if (L->gk_state == GK_TABLES) return 1;
        if (++L->gk_state < GK_BUILD_AT) return 0;
        {
            int k = uaesk_gcm_key_tables(L->stream, &L->c->tb, ks->nr, &ks->ek, L->scratch);
            if (k) return fail(UAES_E_HIP, "key table launch: %s", hipGetErrorString((hipError_t)k));
            L->gk_state = GK_TABLES;
        }
        return 1;
    }
    memset(L->gk, 0, sizeof L->gk);
    memcpy(L->gk, key, kb);
    L->gk_bits = keybits;
    L->gk_state = 1;
    return 0;
}

/* the *_dev entry points do not hold the context lock while the GPU works (they only
 * enqueue), but growing the shared scratch buffer must not race with another thread */
static int gcm_scratch_locked(context *c, void *stream, void **scr, int *slot)
{
    int rc;
    pthread_mutex_lock(&c->mu);
    rc = scratch_pin(c, stream, uaesk_gcm_scratch_bytes(), scr, slot);
    pthread_mutex_unlock(&c->mu);
    return rc;
}

/* enqueue with the pinned scratch, then drop the pin */
#define KCHK_PINNED(c, slot, call)                                                        \
    do {                                                                                  \
        int e_ = (call);                                                                  \
        scratch_unpin((c), (slot));                                                       \
        if (e_ != 0)                                                                      \
            return fail(UAES_E_HIP, "%s failed: %s", #call, hipGetErrorString((hipError_t)e_)); \
    } while (0)

/* AAD may be host memory: stage it (it is read byte-wise, no alignment need) */
static int stage_aad(lane *L, const void *aad, size_t aad_len, const void **d_aad)
{
    *d_aad = aad;
    if (aad_len == 0) { *d_aad = NULL; return 0; }
    if (!aad) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (is_device_ptr(aad)) return wait_for_callers_device_work();
    if (grow_on(L->stream, &L->aad_stage, &L->aad_cap, aad_len + 16)) return UAES_E_HIP;
    /* pageable source: the runtime has copied it out of the caller's buffer when this returns */
    HIPCHK(hipMemcpyAsync(L->aad_stage, aad, aad_len, hipMemcpyHostToDevice, (hipStream_t)L->stream));
    *d_aad = L->aad_stage;
    return 0;
}

/* J0 (GCMsetup, micro_aes.c:1140-1152): nonce || 00000001 for the default 12-byte nonce; for any
 * other length GHASH_H(nonce) computed on the GPU and read back (16 bytes; the counter arithmetic of
 * every kernel is a launch argument).  The lane's scratch has been sized by the caller.          */
static void j0_of_nonce12(const uint8_t *nonce, uint8_t j0[16])
{
    memcpy(j0, nonce, 12);
    j0[12] = j0[13] = j0[14] = 0;
    j0[15] = 1;
}

static int gcm_j0(lane *L, keysched *ks, const uint8_t *nonce, size_t nonce_len, uint8_t j0[16])
{
    const void *d_iv;
    int rc;
    if (nonce_len == 12) { j0_of_nonce12(nonce, j0); return 0; }
    if (nonce_len == 0) return fail(UAES_E_ARG, "empty GCM nonce");
    if ((rc = stage_aad(L, nonce, nonce_len, &d_iv)) != 0) return rc;
    KCHK(uaesk_gcm_j0(L->stream, &L->c->tb, ks->nr, &ks->ek, d_iv, nonce_len, L->scratch, L->d_status + 4));
    return lane_fetch(L, j0, L->d_status + 4, 16);
}

/* A long HOST text through AES_GCM_encrypt: one copy in, the kernels, one copy out use the link one direction at a time.
 * The slice pipeline of ECB / CTR / XTS serves GCM as well since every slice can be a SHARD of the message
 * (uaesk_gcm_shard: CTR at the slice's counter offset fused with the slice's weighted share of the tag, round 5): the
 * workers copy a slice in, run the shard pass on their own stream and scratch, fetch its 16-byte share and copy the
 * slice out; the host XORs the shares into the tag.  Encryption only -- decryption must not release a byte before the
 * whole text has been authenticated (N7), so it keeps the one staging buffer.                                        */
typedef struct {
    context *c; keysched *ks; const uint8_t *nonce; const void *d_aad;
    uint64_t aad_len, total;
    size_t slice;
    uint8_t (*shares)[16];
} gcm_pipe_arg;

static int gcm_pipe_launch(void *arg, int worker, void *stream, const void *d_in, void *d_out, size_t off, size_t len)
{
    gcm_pipe_arg *a = (gcm_pipe_arg *)arg;
    context *c = a->c;
    const size_t sb = uaesk_gcm_scratch_bytes();
    char *scr;
    int k;
    if (grow_on(stream, &c->pipe[worker].xscratch, &c->pipe[worker].xscratch_cap, sb + 64)) return -1;
    scr = (char *)c->pipe[worker].xscratch;
    k = uaesk_gcm_shard(stream, &c->tb, a->ks->nr, &a->ks->ek, 0, a->nonce, off == 0 ? a->d_aad : NULL, a->aad_len,
                        d_in, len, off, a->total, d_out, scr, scr + sb);
    if (k) return k;
    return (int)hipMemcpyAsync(a->shares[off / a->slice], scr + sb, 16, hipMemcpyDeviceToHost, (hipStream_t)stream);
}

/* 1 if the call qualified (then *rc is its result) */
static int gcm_encrypt_pipelined(keysched *ks, const uint8_t *nonce, const void *aData, size_t aDataLen,
                                 const void *pntxt, size_t ptextLen, void *crtxt, int *rc)
{
    context *c;
    lane *L;
    gcm_pipe_arg pa;
    const void *d_aad = NULL;
    size_t slice = pipe_slice_bytes(), nsl, i;
    uint8_t tag[16] = { 0 };
    int k, took;
    if (ptextLen < PIPE_MIN || pipe_workers() < 2 || is_device_ptr(pntxt) || is_device_ptr(crtxt)) return 0;
    slice -= slice % 16;
    if (slice * 2 > ptextLen) return 0;
    if ((*rc = enter(&c, &L)) != 0) return 1;
    /* the AAD once, on the caller's lane, complete before the first worker reads it */
    if ((*rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0 || (*rc = lane_sync(L)) != 0) { *rc = lane_abandon(L, *rc); return 1; }
    nsl = (ptextLen + slice - 1) / slice;
    pa.c = c; pa.ks = ks; pa.nonce = nonce; pa.d_aad = d_aad; pa.aad_len = aDataLen; pa.total = ptextLen; pa.slice = slice;
    pa.shares = (uint8_t (*)[16])calloc(nsl, 16);
    if (!pa.shares) { *rc = fail(UAES_E_HIP, "out of host memory"); return 1; }
    took = run_pipelined(c, pntxt, crtxt, ptextLen, 16, 0, gcm_pipe_launch, &pa, rc);
    if (took && *rc == 0) {
        for (i = 0; i < nsl; ++i)
            for (k = 0; k < 16; ++k) tag[k] ^= pa.shares[i][k];
        memcpy((char *)crtxt + ptextLen, tag, 16);
    }
    free(pa.shares);
    return took;
}

/* nonceLen / tagLen = the reference's compile-time GCM_NONCE_LEN / GCM_TAG_LEN (micro_aes.h:108-109).  The kernels
 * always produce the 16-byte tag behind the text; a shorter tag is the host layer's business: the text goes
 * through a buffer with room for sixteen bytes and ptextLen + tagLen bytes are handed over (:1178).         */
int uaes_gcm_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_aad;
    uint8_t j0[16];
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "GCM tag length %zu (1..16)", tagLen);
    if (nonceLen == 0) return fail(UAES_E_ARG, "empty GCM nonce");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take_mode(pntxt, crtxt, ptextLen, 0, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&ks);
        HOST_RET(ks, uaesh_gcm(&hk, 0, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)pntxt, ptextLen, (uint8_t *)crtxt));
    }
    if (nonceLen == 12 && tagLen == 16) {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(pntxt, crtxt, ptextLen, devs);
        if (nd) return uaes_mgpu_gcm_encrypt(nd, devs, keybits, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
        if (gcm_encrypt_pipelined(&ks, nonce, aData, aDataLen, pntxt, ptextLen, crtxt, &rc)) return rc;
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = gcm_scratch(L, SCRATCH_GCM_KEYED)) != 0) break;
        /* (before anything of this call writes the scratch under its key.  A one-shot setup builds only the tables its
         * message reaches and leaves the others undefined: with a nonce whose J0 is a GHASH of its own, which runs such
         * a setup, the call stays one-shot and the cache starts over) */
        int keyed = nonceLen == 12 ? lane_gcm_keyed(L, &ks, key, keybits) : 0;
        if (keyed < 0) { rc = keyed; break; }
        if (nonceLen != 12) lane_scratch_clobbered(L);
        if ((rc = gcm_j0(L, &ks, nonce, nonceLen, j0)) != 0) break;
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, pntxt, ptextLen, crtxt, ptextLen + tagLen, &io)) != 0) break;
        if (tagLen < 16 && io.dout == crtxt) {
            /* the caller's own device buffer ends tagLen bytes behind the text: run into staging, copy back */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], ptextLen + 64)) { rc = UAES_E_HIP; break; }
            io.dout = L->stage[1];
            io.copy_back = 1;
        }
        ticket_arm(L, ptextLen);
        arm_done_word(scratch_done_word(L->scratch, L->scratch_cap));
        int k = keyed ? uaesk_gcm_keyed(L->stream, &c->tb, ks.nr, &ks.ek, 0, j0, d_aad, aDataLen,
                                        io.din, ptextLen, io.dout, L->scratch, NULL)
                      : uaesk_gcm(L->stream, &c->tb, ks.nr, &ks.ek, 0, j0, d_aad, aDataLen,
                                  io.din, ptextLen, io.dout, L->scratch, NULL);
        arm_done_word(NULL);
        ticket_armed_launch_done(L);
        if (k) { rc = fail(UAES_E_HIP, "gcm launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, ptextLen + tagLen);
    } while (0);
    DONE(L, rc);
}

int uaes_gcm_encrypt_iv(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    return uaes_gcm_encrypt_ex(keybits, key, nonce, nonceLen, 16, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_gcm_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, void *crtxt)
{
    return uaes_gcm_encrypt_iv(keybits, key, nonce, 12, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_gcm_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_aad;
    uint8_t j0[16];
    int rc, status = -1;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !crtxt || (crtxtLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "GCM tag length %zu (1..16)", tagLen);
    if (nonceLen == 0) return fail(UAES_E_ARG, "empty GCM nonce");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take_mode(crtxt, pntxt, crtxtLen, 0, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&ks);
        HOST_RET(ks, uaesh_gcm(&hk, 1, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)crtxt, crtxtLen, (uint8_t *)pntxt));
    }
    if (nonceLen == 12 && tagLen == 16) {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(crtxt, pntxt, crtxtLen, devs);
        if (nd) return uaes_mgpu_gcm_decrypt(nd, devs, keybits, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = gcm_scratch(L, SCRATCH_GCM_KEYED)) != 0) break;
        /* (before anything of this call writes the scratch under its key.  A one-shot setup builds only the tables its
         * message reaches and leaves the others undefined: with a nonce whose J0 is a GHASH of its own, which runs such
         * a setup, the call stays one-shot and the cache starts over) */
        int keyed = nonceLen == 12 ? lane_gcm_keyed(L, &ks, key, keybits) : 0;
        if (keyed < 0) { rc = keyed; break; }
        if (nonceLen != 12) lane_scratch_clobbered(L);
        if ((rc = gcm_j0(L, &ks, nonce, nonceLen, j0)) != 0) break;
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        /* input is CT || tag; output is crtxtLen bytes */
        if ((rc = plan_io(L, crtxt, crtxtLen + tagLen, pntxt, crtxtLen, &io)) != 0) break;
        if (tagLen < 16) {
            /* a truncated tag (GCM_TAG_LEN < 16, :1204) is compared here: the device computes the full tag of the
             * ciphertext (nothing is decrypted), its first tagLen bytes are checked against the ones behind the
             * text in constant time, and only then does the CTR pass write the caller's buffer (N7)          */
            uint8_t full[16], given[16];
            int k = keyed ? uaesk_gcm_keyed(L->stream, &c->tb, ks.nr, &ks.ek, 3, j0, d_aad, aDataLen,
                                            io.din, crtxtLen, NULL, L->scratch, L->d_status + 4)
                          : uaesk_gcm(L->stream, &c->tb, ks.nr, &ks.ek, 3, j0, d_aad, aDataLen,
                                      io.din, crtxtLen, NULL, L->scratch, L->d_status + 4);
            if (k) { rc = fail(UAES_E_HIP, "gcm launch: %s", hipGetErrorString((hipError_t)k)); break; }
            if ((rc = lane_fetch(L, full, L->d_status + 4, 16)) != 0) break;
            if (is_device_ptr(io.din)) {
                if (hipMemcpy(given, (const char *)io.din + crtxtLen, tagLen, hipMemcpyDeviceToHost) != hipSuccess) {
                    rc = fail(UAES_E_HIP, "reading the tag back failed");
                    break;
                }
            } else {
                memcpy(given, (const char *)io.din + crtxtLen, tagLen);     /* the mapped pinned window */
            }
            if (tags_differ(full, given, tagLen)) { rc = UAES_E_AUTHENTICATION; break; }
            k = uaesk_gcm_ctr(L->stream, &c->tb, ks.nr, &ks.ek, j0, io.din, crtxtLen, io.dout);
            if (k) { rc = fail(UAES_E_HIP, "gcm launch: %s", hipGetErrorString((hipError_t)k)); break; }
            rc = finish_io(&io, crtxtLen);
            break;
        }
        if (io.dout == io.din && io.copy_back) {
            /* host -> host: decrypt into the second staging buffer so that a
             * failed authentication can leave the caller's buffer untouched   */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], crtxtLen + 64)) { rc = UAES_E_HIP; break; }
            io.dout = L->stage[1];
        }
        /* a private staging buffer may be written before the tag is known: one pass */
        int *st_where = lane_status(L);
        if (st_where != L->d_status) { *(volatile int *)st_where = -1; ticket_arm(L, crtxtLen); }   /* host-visible status: a
                                                     * one-launch decryption may carry the completion ticket itself */
        arm_done_word(scratch_done_word(L->scratch, L->scratch_cap));
        const int dmode = io.copy_back || io.dout == L->pin[1] ? 2 : gcm_decrypt_mode();
        int k = keyed ? uaesk_gcm_keyed(L->stream, &c->tb, ks.nr, &ks.ek, dmode, j0, d_aad, aDataLen, io.din, crtxtLen, io.dout,
                                        L->scratch, st_where)
                      : uaesk_gcm(L->stream, &c->tb, ks.nr, &ks.ek, dmode, j0, d_aad, aDataLen, io.din, crtxtLen, io.dout,
                                  L->scratch, st_where);
        arm_done_word(NULL);
        ticket_armed_launch_done(L);
        if (k) { rc = fail(UAES_E_HIP, "gcm launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if ((rc = lane_read_status(L, st_where, &status)) != 0) break;
        if (status != 0) { rc = UAES_E_AUTHENTICATION; break; }  /* N7: pntxt untouched */
        io.drained = 1;
        rc = finish_io(&io, crtxtLen);
    } while (0);
    DONE(L, rc);
}

int uaes_gcm_decrypt_iv(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return uaes_gcm_decrypt_ex(keybits, key, nonce, nonceLen, 16, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

int uaes_gcm_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return uaes_gcm_decrypt_iv(keybits, key, nonce, 12, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

int uaes_gcm_encrypt_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, size_t aad_len,
                         const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    keysched ks;
    void *scr;
    uint8_t j0[16];
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !d_out) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    j0_of_nonce12(nonce, j0);
    arm_done_word(scratch_done_word(scr, c->slot[slot].cap));
    rc = uaesk_gcm(stream, &c->tb, ks.nr, &ks.ek, 0, j0, d_aad, aad_len, d_in, len, d_out, scr, NULL);
    disarm_done_word_dev(stream, rc);
    KCHK_PINNED(c, slot, rc);
    return 0;
}

int uaes_gcm_decrypt_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, size_t aad_len,
                         const void *d_in, size_t len, void *d_out,
                         int *d_status, void *stream)
{
    context *c;
    keysched ks;
    void *scr;
    uint8_t j0[16];
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !d_in) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if (!d_status) return fail(UAES_E_ARG, "NULL d_status");
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    j0_of_nonce12(nonce, j0);
    arm_done_word(scratch_done_word(scr, c->slot[slot].cap));
    rc = uaesk_gcm(stream, &c->tb, ks.nr, &ks.ek, gcm_decrypt_mode(), j0, d_aad, aad_len, d_in, len, d_out, scr, d_status);
    disarm_done_word_dev(stream, rc);
    KCHK_PINNED(c, slot, rc);
    return 0;
}

/* ------------------------------------------------------------------------ */
/* GCM key context: the tables of a key built once                             */
/* ------------------------------------------------------------------------ */
struct uaes_gcm_key {
    keysched ks;
    int      device;
    void    *scratch;               /* uaesk_gcm_scratch_bytes(): the key's tables + per-message state, then SCRATCH_TAIL bytes
                                     * of zero-between-calls words like the lanes' scratch buffers have */
};
#define KEY_DONE_WORD(k) ((unsigned *)((char *)(k)->scratch + uaesk_gcm_scratch_bytes()))

int uaes_gcm_key_new(uaes_gcm_key **out, int keybits, const uint8_t *key)
{
    context *c;
    lane *L;
    uaes_gcm_key *k;
    int rc;
    if (!out) return fail(UAES_E_ARG, "NULL pointer");
    *out = NULL;
    if ((k = (uaes_gcm_key *)calloc(1, sizeof *k)) == NULL) return fail(UAES_E_HIP, "out of host memory");
    /* every way out below wipes the expanded key before the memory goes back to the allocator */
    if ((rc = expand_key(&k->ks, key, keybits)) != 0 || (rc = enter(&c, &L)) != 0) {
        memset(k, 0, sizeof *k);
        free(k);
        return rc;
    }
    if (hipGetDevice(&k->device) != hipSuccess) rc = fail(UAES_E_HIP, "hipGetDevice failed");
    else if (hipMalloc(&k->scratch, uaesk_gcm_scratch_bytes() + SCRATCH_TAIL) != hipSuccess) {
        k->scratch = NULL;
        rc = fail(UAES_E_HIP, "key context allocation failed (%zu bytes of device memory)", uaesk_gcm_scratch_bytes());
    }
    if (rc == 0 && hipMemsetAsync(KEY_DONE_WORD(k), 0, SCRATCH_TAIL, (hipStream_t)L->stream) != hipSuccess)
        rc = fail(UAES_E_HIP, "key context: hipMemsetAsync failed");
    if (rc == 0) {
        int kk = uaesk_gcm_key_tables(L->stream, &c->tb, k->ks.nr, &k->ks.ek, k->scratch);
        if (kk) rc = fail(UAES_E_HIP, "key table launch: %s", hipGetErrorString((hipError_t)kk));
        else if (hipStreamSynchronize((hipStream_t)L->stream) != hipSuccess) rc = fail(UAES_E_HIP, "key table build failed");
    }
    if (rc) {
        if (k->scratch) (void)hipFree(k->scratch);
        memset(k, 0, sizeof *k);
        free(k);
        return rc;
    }
    *out = k;
    return 0;
}

void uaes_gcm_key_free(uaes_gcm_key *k)
{
    if (!k) return;
    if (k->scratch) {
        (void)hipDeviceSynchronize();
        (void)hipMemset(k->scratch, 0, uaesk_gcm_scratch_bytes());    /* H and its tables are key material */
        (void)hipFree(k->scratch);
    }
    memset(k, 0, sizeof *k);
    free(k);
}

static int key_device_ok(const uaes_gcm_key *k)
{
    int dev = -1;
    if (!k) return fail(UAES_E_ARG, "NULL key context");
    if (hipGetDevice(&dev) != hipSuccess || dev != k->device)
        return fail(UAES_E_ARG, "the key context belongs to device %d, the calling thread is bound to %d", k->device, dev);
    return 0;
}

int uaes_gcm_key_encrypt(uaes_gcm_key *k, const uint8_t *nonce, const void *aData, size_t aDataLen,
                         const void *pntxt, size_t ptextLen, void *crtxt)
{
    context *c;
    lane *L;
    io_plan io;
    const void *d_aad;
    uint8_t j0[16];
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    j0_of_nonce12(nonce, j0);
    do {
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, pntxt, ptextLen, crtxt, ptextLen + 16, &io)) != 0) break;
        ticket_arm(L, ptextLen);
        arm_done_word(KEY_DONE_WORD(k));
        int kk = uaesk_gcm_keyed(L->stream, &c->tb, k->ks.nr, &k->ks.ek, 0, j0, d_aad, aDataLen,
                                 io.din, ptextLen, io.dout, k->scratch, NULL);
        arm_done_word(NULL);
        ticket_armed_launch_done(L);
        if (kk) { rc = fail(UAES_E_HIP, "gcm launch: %s", hipGetErrorString((hipError_t)kk)); break; }
        rc = finish_io(&io, ptextLen + 16);
    } while (0);
    DONE(L, rc);
}

int uaes_gcm_key_decrypt(uaes_gcm_key *k, const uint8_t *nonce, const void *aData, size_t aDataLen,
                         const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    io_plan io;
    const void *d_aad;
    uint8_t j0[16];
    int rc, status = -1;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !crtxt || (crtxtLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    j0_of_nonce12(nonce, j0);
    do {
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, crtxt, crtxtLen + 16, pntxt, crtxtLen, &io)) != 0) break;
        if (io.dout == io.din && io.copy_back) {      /* host -> host: keep the caller's buffer untouched on 0x1A */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], crtxtLen + 64)) { rc = UAES_E_HIP; break; }
            io.dout = L->stage[1];
        }
        int *st_where = lane_status(L);
        if (st_where != L->d_status) { *(volatile int *)st_where = -1; ticket_arm(L, crtxtLen); }
        arm_done_word(KEY_DONE_WORD(k));
        int kk = uaesk_gcm_keyed(L->stream, &c->tb, k->ks.nr, &k->ks.ek,
                                 io.copy_back || io.dout == L->pin[1] ? 2 : gcm_decrypt_mode(), j0, d_aad, aDataLen,
                                 io.din, crtxtLen, io.dout, k->scratch, st_where);
        arm_done_word(NULL);
        ticket_armed_launch_done(L);
        if (kk) { rc = fail(UAES_E_HIP, "gcm launch: %s", hipGetErrorString((hipError_t)kk)); break; }
        if ((rc = lane_read_status(L, st_where, &status)) != 0) break;
        if (status != 0) { rc = UAES_E_AUTHENTICATION; break; }  /* N7: pntxt untouched */
        io.drained = 1;
        rc = finish_io(&io, crtxtLen);
    } while (0);
    DONE(L, rc);
}

int uaes_gcm_key_encrypt_dev(uaes_gcm_key *k, const uint8_t *nonce, const void *d_aad, size_t aad_len,
                             const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    uint8_t j0[16];
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !d_out) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    j0_of_nonce12(nonce, j0);
    arm_done_word(KEY_DONE_WORD(k));
    rc = uaesk_gcm_keyed(stream, &c->tb, k->ks.nr, &k->ks.ek, 0, j0, d_aad, aad_len, d_in, len, d_out, k->scratch, NULL);
    disarm_done_word_dev(stream, rc);
    KCHK(rc);
    return 0;
}

int uaes_gcm_key_decrypt_dev(uaes_gcm_key *k, const uint8_t *nonce, const void *d_aad, size_t aad_len,
                             const void *d_in, size_t len, void *d_out, int *d_status, void *stream)
{
    context *c;
    uint8_t j0[16];
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !d_in || !d_status) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    j0_of_nonce12(nonce, j0);
    arm_done_word(KEY_DONE_WORD(k));
    rc = uaesk_gcm_keyed(stream, &c->tb, k->ks.nr, &k->ks.ek, gcm_decrypt_mode(), j0, d_aad, aad_len, d_in, len, d_out, k->scratch, d_status);
    disarm_done_word_dev(stream, rc);
    KCHK(rc);
    return 0;
}

/* ---- many short messages under one key context in one launch (uaesk_gcm_records) -------------------------
 * The reference has one message per call (AES_GCM_encrypt, micro_aes.c:1164-1179); a call costs ~12 us on this
 * engine whatever the size, so record streams (TLS records, packets, pages) come as one call: record r is rec_len
 * bytes at in + r * in_stride under the 12-byte nonce nonces + 12 r, with the AAD at aad + r * aad_stride (stride
 * 0: one AAD for all).  Each record's result is exactly what uaes_gcm_key_encrypt / _decrypt give for it.  */
size_t uaes_gcm_record_max(size_t aad_len)
{
    return uaesk_gcm_record_max(aad_len);
}

static int records_args_ok(size_t nrec, const void *nonces, const void *aad, size_t aad_len,
                           const void *in, size_t rec_len, size_t in_stride, size_t in_min,
                           const void *out, size_t out_stride, size_t out_min)
{
    if (!nrec) return 0;
    if (!nonces || !in || !out || (aad_len && !aad)) return fail(UAES_E_ARG, "NULL pointer");
    if (rec_len > uaesk_gcm_record_max(aad_len))
        return fail(UAES_E_ARG, "a record of %zu bytes with %zu bytes of AAD is too long for the record call (%zu)",
                    rec_len, aad_len, uaesk_gcm_record_max(aad_len));
    if ((in_stride | out_stride) & 15u) return fail(UAES_E_ARG, "record strides must be multiples of 16");
    if (in_stride < in_min || out_stride < out_min) return fail(UAES_E_ARG, "record stride shorter than a record");
    if (nrec > (size_t)1 << 40 || in_stride > (size_t)1 << 22 || out_stride > (size_t)1 << 22)
        return fail(UAES_E_ARG, "too many records / record stride too long");     /* spans stay far below 2^64 */
    return 0;
}

static int records_enc_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                           const void *d_aad, size_t aad_len, size_t aad_stride,
                           const void *d_in, const uint32_t *d_lens, size_t rec_len, size_t in_stride,
                           void *d_out, size_t out_stride, void *stream)
{
    context *c;
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if ((rc = records_args_ok(nrec, d_nonces, d_aad, aad_len, d_in, rec_len, in_stride, rec_len,
                              d_out, out_stride, rec_len + 16)) != 0) return rc;
    if ((rc = dev_ptrs_ok(d_in, d_out, 1)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    KCHK(uaesk_gcm_records(stream, &c->tb, k->ks.nr, &k->ks.ek, 0, d_nonces, d_aad, aad_len, aad_stride,
                           d_in, rec_len, in_stride, d_out, out_stride, nrec, k->scratch, NULL, NULL, d_lens));
    return 0;
}

int uaes_gcm_key_encrypt_records_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                     const void *d_aad, size_t aad_len, size_t aad_stride,
                                     const void *d_in, size_t rec_len, size_t in_stride,
                                     void *d_out, size_t out_stride, void *stream)
{
    return records_enc_dev(k, nrec, d_nonces, d_aad, aad_len, aad_stride, d_in, NULL, rec_len, in_stride, d_out, out_stride, stream);
}

int uaes_gcm_key_encrypt_records_v_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                       const void *d_aad, size_t aad_len, size_t aad_stride,
                                       const void *d_in, const uint32_t *d_lens, size_t max_len, size_t in_stride,
                                       void *d_out, size_t out_stride, void *stream)
{
    if (nrec && !d_lens) return fail(UAES_E_ARG, "NULL lengths");
    return records_enc_dev(k, nrec, d_nonces, d_aad, aad_len, aad_stride, d_in, d_lens, max_len, in_stride, d_out, out_stride, stream);
}

static int records_dec_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                           const void *d_aad, size_t aad_len, size_t aad_stride,
                           const void *d_in, const uint32_t *d_lens, size_t rec_len, size_t in_stride,
                           void *d_out, size_t out_stride, uint8_t *d_verdicts, int *d_status, void *stream)
{
    context *c;
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!d_status) return fail(UAES_E_ARG, "NULL d_status");
    if ((rc = records_args_ok(nrec, d_nonces, d_aad, aad_len, d_in, rec_len, in_stride, rec_len + 16,
                              d_out, out_stride, rec_len)) != 0) return rc;
    if ((rc = dev_ptrs_ok(d_in, d_out, 1)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int), (hipStream_t)stream));
    KCHK(uaesk_gcm_records(stream, &c->tb, k->ks.nr, &k->ks.ek, 1, d_nonces, d_aad, aad_len, aad_stride,
                           d_in, rec_len, in_stride, d_out, out_stride, nrec, k->scratch, d_verdicts, d_status, d_lens));
    return 0;
}

int uaes_gcm_key_decrypt_records_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                     const void *d_aad, size_t aad_len, size_t aad_stride,
                                     const void *d_in, size_t rec_len, size_t in_stride,
                                     void *d_out, size_t out_stride, uint8_t *d_verdicts, int *d_status, void *stream)
{
    return records_dec_dev(k, nrec, d_nonces, d_aad, aad_len, aad_stride, d_in, NULL, rec_len, in_stride, d_out, out_stride,
                           d_verdicts, d_status, stream);
}

int uaes_gcm_key_decrypt_records_v_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                       const void *d_aad, size_t aad_len, size_t aad_stride,
                                       const void *d_in, const uint32_t *d_lens, size_t max_len, size_t in_stride,
                                       void *d_out, size_t out_stride, uint8_t *d_verdicts, int *d_status, void *stream)
{
    if (nrec && !d_lens) return fail(UAES_E_ARG, "NULL lengths");
    return records_dec_dev(k, nrec, d_nonces, d_aad, aad_len, aad_stride, d_in, d_lens, max_len, in_stride, d_out, out_stride,
                           d_verdicts, d_status, stream);
}

/* host (or device) pointers, synchronous: nonces and AAD go through the lane's AAD staging, the texts through its
 * two text stagings; only the records' own bytes are written to the caller's output (the gaps of a strided layout,
 * and on decryption the records whose tag is wrong -- N7 -- keep what they held) */
static int records_sync(uaes_gcm_key *k, int decrypt, size_t nrec, const uint8_t *nonces,
                        const void *aad, size_t aad_len, size_t aad_stride,
                        const void *in, const uint32_t *lens, size_t rec_len, size_t in_stride,
                        void *out, size_t out_stride, uint8_t *verdicts)
{
    context *c;
    lane *L;
    int rc;
    const size_t in_rec = rec_len + (decrypt ? 16 : 0), out_rec = rec_len + (decrypt ? 0 : 16);
    if ((rc = key_device_ok(k)) != 0) return rc;
    if ((rc = records_args_ok(nrec, nonces, aad, aad_len, in, rec_len, in_stride, in_rec, out, out_stride, out_rec)) != 0)
        return rc;
    if (!nrec) return 0;
    if (aad_len && aad_stride && aad_stride < aad_len) return fail(UAES_E_ARG, "AAD stride shorter than the AAD");
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        hipStream_t st = (hipStream_t)L->stream;
        const size_t non_span = (12 * nrec + 15) & ~(size_t)15;
        const size_t aad_span = aad_len ? (aad_stride ? (nrec - 1) * aad_stride + aad_len : aad_len) : 0;
        const size_t lens_off = non_span + ((aad_span + 15) & ~(size_t)15), lens_span = lens ? 4 * nrec : 0;
        const size_t in_span = (nrec - 1) * in_stride + in_rec, out_span = (nrec - 1) * out_stride + out_rec;
        const size_t ver_off = (out_span + 15) & ~(size_t)15;
        const int in_place = in == out && in_stride == out_stride;
        unsigned char *d_meta, *d_out, *d_ver;
        const unsigned char *d_in;
        int status = 0;
        if (is_device_ptr(nonces) || is_device_ptr(aad) || is_device_ptr(in) || is_device_ptr(out) || is_device_ptr(lens))
            if ((rc = wait_for_callers_device_work()) != 0) break;
        if (lens && !is_device_ptr(lens)) {                   /* (the kernel clamps; a host array can be checked here) */
            size_t r;
            for (r = 0; r < nrec && lens[r] <= rec_len; ++r) { }
            if (r < nrec) { rc = fail(UAES_E_ARG, "record %zu is %u bytes, longer than max_len %zu", r, lens[r], rec_len); break; }
        }
        if (grow_on(st, &L->aad_stage, &L->aad_cap, lens_off + lens_span + 16)) { rc = UAES_E_HIP; break; }
        d_meta = (unsigned char *)L->aad_stage;
        if (hipMemcpyAsync(d_meta, nonces, 12 * nrec, hipMemcpyDefault, st) != hipSuccess ||
            (aad_span && hipMemcpyAsync(d_meta + non_span, aad, aad_span, hipMemcpyDefault, st) != hipSuccess) ||
            (lens_span && hipMemcpyAsync(d_meta + lens_off, lens, lens_span, hipMemcpyDefault, st) != hipSuccess)) {
            rc = fail(UAES_E_HIP, "staging the nonces failed");
            break;
        }
        if (grow_on(st, &L->stage[0], &L->stage_cap[0], in_span + 64)) { rc = UAES_E_HIP; break; }
        if (hipMemcpyAsync(L->stage[0], in, in_span, hipMemcpyDefault, st) != hipSuccess) {
            rc = fail(UAES_E_HIP, "staging the records failed");
            break;
        }
        d_in = (const unsigned char *)L->stage[0];
        /* the output staging also holds the verdict bytes behind the records */
        if (in_place && !decrypt) {
            d_out = (unsigned char *)L->stage[0];             /* sized in_span + 64: the last tag fits */
            d_ver = NULL;
        } else {
            if (grow_on(st, &L->stage[1], &L->stage_cap[1], ver_off + nrec + 64)) { rc = UAES_E_HIP; break; }
            d_out = (unsigned char *)L->stage[1];
            d_ver = d_out + ver_off;
            /* variable-length records: the kernel writes lens[r] (+16) bytes of a slot and whole slots are copied
             * back, so what lies between must not be whatever an earlier call of this thread left in the staging
             * buffer (another message's plaintext): the slots' tails come back as zeros */
            if (lens && hipMemsetAsync(d_out, 0, out_span, st) != hipSuccess) { rc = fail(UAES_E_HIP, "memset failed"); break; }
        }
        if (decrypt && hipMemsetAsync(L->d_status, 0, sizeof(int), st) != hipSuccess) { rc = fail(UAES_E_HIP, "memset failed"); break; }
        {
            int kk = uaesk_gcm_records(L->stream, &c->tb, k->ks.nr, &k->ks.ek, decrypt, d_meta,
                                       aad_span ? d_meta + non_span : NULL, aad_len, aad_stride, d_in, rec_len, in_stride,
                                       d_out, out_stride, nrec, k->scratch, decrypt ? d_ver : NULL, decrypt ? L->d_status : NULL,
                                       lens ? d_meta + lens_off : NULL);
            if (kk) { rc = fail(UAES_E_HIP, "gcm records launch: %s", hipGetErrorString((hipError_t)kk)); break; }
        }
        if (decrypt) {
            if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) break;
            if (verdicts || status) {
                uint8_t *v = verdicts;
                if (!v && (v = (uint8_t *)malloc(nrec)) == NULL) { rc = fail(UAES_E_HIP, "out of host memory"); break; }
                if (hipMemcpyAsync(v, d_ver, nrec, hipMemcpyDefault, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                    if (v != verdicts) free(v);
                    rc = fail(UAES_E_HIP, "verdict copy failed");
                    break;
                }
                if (status) {                                 /* the good records (N7 for the others): runs of consecutive
                                                               * good records go back as one 2-D copy each */
                    const int host_lens = lens && !is_device_ptr(lens);
                    size_t r = 0;
                    while (r < nrec && rc == 0 && rec_len) {
                        size_t e;
                        if (v[r]) { ++r; continue; }
                        if (host_lens) {                       /* exactly lens[r] bytes each: one record per copy */
                            if (lens[r] && hipMemcpyAsync((char *)out + r * out_stride, d_out + r * out_stride, lens[r],
                                                          hipMemcpyDefault, st) != hipSuccess)
                                rc = fail(UAES_E_HIP, "copy back failed");
                            ++r;
                            continue;
                        }
                        for (e = r + 1; e < nrec && v[e] == 0; ++e) { }
                        if (hipMemcpy2DAsync((char *)out + r * out_stride, out_stride, d_out + r * out_stride, out_stride,
                                             rec_len, e - r, hipMemcpyDefault, st) != hipSuccess)
                            rc = fail(UAES_E_HIP, "copy back failed");
                        r = e;
                    }
                    if (v != verdicts) free(v);
                    if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = fail(UAES_E_HIP, "copy back failed");
                    if (rc == 0) rc = UAES_E_AUTHENTICATION;
                    break;
                }
                if (v != verdicts) free(v);
            }
        }
        if (out_rec && hipMemcpy2DAsync(out, out_stride, d_out, out_stride, out_rec, nrec, hipMemcpyDefault, st) != hipSuccess) {
            rc = fail(UAES_E_HIP, "copy back failed");
            break;
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc = fail(UAES_E_HIP, "gcm records failed");
    } while (0);
    DONE(L, rc);
}

int uaes_gcm_key_encrypt_records(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                 const void *aad, size_t aad_len, size_t aad_stride,
                                 const void *in, size_t rec_len, size_t in_stride, void *out, size_t out_stride)
{
    return records_sync(k, 0, nrec, nonces, aad, aad_len, aad_stride, in, NULL, rec_len, in_stride, out, out_stride, NULL);
}

int uaes_gcm_key_decrypt_records(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                 const void *aad, size_t aad_len, size_t aad_stride,
                                 const void *in, size_t rec_len, size_t in_stride, void *out, size_t out_stride,
                                 uint8_t *verdicts)
{
    return records_sync(k, 1, nrec, nonces, aad, aad_len, aad_stride, in, NULL, rec_len, in_stride, out, out_stride, verdicts);
}

/* records of DIFFERENT lengths in slots of one size (packet buffers): record r is lens[r] <= max_len bytes at the start of
 * its slot, its tag follows its own text.  What else of a slot's first max_len + 16 output bytes holds afterwards is
 * unspecified, but never another call's data: the synchronous flavour copies whole slots back from a staging buffer
 * whose slots were zeroed before the launch, so the tail of a slot reads as zeros. */
int uaes_gcm_key_encrypt_records_v(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                   const void *aad, size_t aad_len, size_t aad_stride,
                                   const void *in, const uint32_t *lens, size_t max_len, size_t in_stride,
                                   void *out, size_t out_stride)
{
    if (nrec && !lens) return fail(UAES_E_ARG, "NULL lengths");
    return records_sync(k, 0, nrec, nonces, aad, aad_len, aad_stride, in, lens, max_len, in_stride, out, out_stride, NULL);
}

int uaes_gcm_key_decrypt_records_v(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                   const void *aad, size_t aad_len, size_t aad_stride,
                                   const void *in, const uint32_t *lens, size_t max_len, size_t in_stride,
                                   void *out, size_t out_stride, uint8_t *verdicts)
{
    if (nrec && !lens) return fail(UAES_E_ARG, "NULL lengths");
    return records_sync(k, 1, nrec, nonces, aad, aad_len, aad_stride, in, lens, max_len, in_stride, out, out_stride, verdicts);
}

int uaes_gcm_partial_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, uint64_t total_aad_len,
                         const void *d_ct_shard, size_t shard_len, uint64_t shard_offset,
                         uint64_t total_len, void *d_partial16, void *stream)
{
    context *c;
    keysched ks;
    void *scr;
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !d_partial16) return fail(UAES_E_ARG, "NULL pointer");
    if (((uintptr_t)d_ct_shard) & 15u) return fail(UAES_E_ARG, "the ciphertext shard must be 16-byte aligned");
    if (shard_offset % 16 || shard_offset + shard_len > total_len)
        return fail(UAES_E_ARG, "shard [%llu, +%zu) is not a 16-byte aligned slice of %llu bytes",
                    (unsigned long long)shard_offset, shard_len, (unsigned long long)total_len);
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    KCHK_PINNED(c, slot, uaesk_gcm_partial(stream, &c->tb, ks.nr, &ks.ek, nonce, d_aad, total_aad_len,
                                           d_ct_shard, shard_len, shard_offset, total_len, scr, d_partial16));
    return 0;
}

/* the shard's CTR pass and its share in ONE pass on the caller's stream (uaesk_gcm_shard): what a rank of a
 * one-process-per-GPU job runs on its slice of one GCM message */
int uaes_gcm_shard_dev(int keybits, const uint8_t *key, const uint8_t *nonce, int mode,
                       const void *d_aad, uint64_t total_aad_len,
                       const void *d_in, size_t shard_len, uint64_t shard_offset, uint64_t total_len,
                       void *d_out, void *d_partial16, void *stream)
{
    context *c;
    keysched ks;
    void *scr;
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !d_partial16) return fail(UAES_E_ARG, "NULL pointer");
    if (mode < 0 || mode > 2) return fail(UAES_E_ARG, "mode %d (0 encrypt, 1 hash only, 2 decrypt)", mode);
    if ((((uintptr_t)d_in) | ((uintptr_t)(mode == 1 ? NULL : d_out))) & 15u)
        return fail(UAES_E_ARG, "the shard buffers must be 16-byte aligned");
    if (shard_len && (!d_in || (mode != 1 && !d_out))) return fail(UAES_E_ARG, "NULL shard buffer");
    if (shard_offset % 16 || shard_offset + shard_len > total_len || (shard_len % 16 && shard_offset + shard_len != total_len))
        return fail(UAES_E_ARG, "shard [%llu, +%zu) is not a 16-byte aligned slice of %llu bytes",
                    (unsigned long long)shard_offset, shard_len, (unsigned long long)total_len);
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    KCHK_PINNED(c, slot, uaesk_gcm_shard(stream, &c->tb, ks.nr, &ks.ek, mode, nonce, d_aad, total_aad_len,
                                         d_in, shard_len, shard_offset, total_len, d_out, scr, d_partial16));
    return 0;
}

int uaes_ghash(const uint8_t H[16], const void *aData, size_t aDataLen,
               const void *crtxt, size_t crtxtLen, uint8_t gh[16])
{
    context *c;
    lane *L;
    io_plan io;
    const void *d_aad;
    int rc;
    if (!H || !gh) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = gcm_scratch(L, SCRATCH_OTHER)) != 0) break;
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, crtxt, crtxtLen, NULL, 0, &io)) != 0) break;
        int k = uaesk_ghash(L->stream, &c->tb, H, d_aad, aDataLen, io.din, crtxtLen, L->scratch, L->d_status + 4);
        if (k) { rc = fail(UAES_E_HIP, "ghash launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = lane_fetch(L, gh, L->d_status + 4, 16);
    } while (0);
    DONE(L, rc);
}

/* ------------------------------------------------------------------------ */
/* CMAC and CCM: serial CBC-MAC chains, one GPU lane */
/* ------------------------------------------------------------------------ */
int uaes_cmac(int keybits, const uint8_t *key, const void *data, size_t dataSize, uint8_t mac[16])
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!mac || (dataSize && !data)) return fail(UAES_E_ARG, "NULL pointer");
    if (host_take(data, NULL, dataSize, 1)) {
        const uaesh_key hk = host_key(&ks);
        uaesh_cmac(&hk, (const uint8_t *)data, dataSize, mac);
        HOST_RET(ks, 0);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = plan_io(L, data, dataSize, NULL, 0, &io)) != 0) break;
        int k = uaesk_cmac(L->stream, &c->tb, ks.nr, &ks.ek, io.din, dataSize, L->d_status + 4);
        if (k) { rc = fail(UAES_E_HIP, "cmac launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = lane_fetch(L, mac, L->d_status + 4, 16);
    } while (0);
    DONE(L, rc);
}

/* ------------------------------------------------------------------------ */
/* Poly1305-AES (micro_aes.c:1901-1997): keys = k (keybits / 8 bytes) || r (16) */
/* ------------------------------------------------------------------------ */
/* AES_k(nonce), the powers of r and the tag run in kernels (uaes_poly1305.hip); the host expands k, and the clamped r
 * travels as a launch argument.  Every way out wipes the schedule; the chunk partials are zeroed by the fold kernel. */
int uaes_poly1305(int keybits, const uint8_t *keys, const uint8_t nonce[16],
                  const void *data, size_t dataSize, uint8_t mac[16])
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    int rc;
    if (!keys || !nonce || !mac || (dataSize && !data)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&ks, keys, keybits)) != 0) return rc;
    const uint8_t *r = keys + keybits / 8;
    if (host_take(data, NULL, dataSize, 0)) {
        const uaesh_key hk = host_key(&ks);
        uaesh_poly1305(&hk, r, nonce, (const uint8_t *)data, dataSize, mac);
        HOST_RET(ks, 0);
    }
    if ((rc = enter(&c, &L)) != 0) { burn(&ks, sizeof ks); return rc; }
    do {
        const size_t need = uaesk_poly1305_scratch_bytes(dataSize);
        if ((rc = plan_io(L, data, dataSize, NULL, 0, &io)) != 0) break;
        if (need && (rc = lane_scratch(L, need, SCRATCH_OTHER)) != 0) break;
        int k = uaesk_poly1305(L->stream, &c->tb, ks.nr, &ks.ek, r, nonce, io.din, dataSize, L->d_status + 4,
                               need ? L->scratch : NULL);
        if (k) { rc = fail(UAES_E_HIP, "poly1305 launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = lane_fetch(L, mac, L->d_status + 4, 16);
    } while (0);
    burn(&ks, sizeof ks);
    DONE(L, rc);
}

int uaes_poly1305_dev(int keybits, const uint8_t *keys, const uint8_t nonce[16],
                      const void *d_data, size_t len, void *d_mac, void *stream)
{
    context *c;
    keysched ks;
    void *scr = NULL;
    int rc, slot = -1;
    if (!keys || !nonce || !d_mac || (len && !d_data)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&ks, keys, keybits)) != 0) return rc;
    const size_t need = uaesk_poly1305_scratch_bytes(len);
    if ((rc = get_context(&c)) != 0) { burn(&ks, sizeof ks); return rc; }
    if (need) {
        pthread_mutex_lock(&c->mu);
        rc = scratch_pin(c, stream, need, &scr, &slot);
        pthread_mutex_unlock(&c->mu);
        if (rc) { burn(&ks, sizeof ks); return fail(UAES_E_HIP, "poly1305 scratch"); }
    }
    rc = uaesk_poly1305(stream, &c->tb, ks.nr, &ks.ek, keys + keybits / 8, nonce, d_data, len, d_mac, scr);
    burn(&ks, sizeof ks);
    KCHK_PINNED(c, slot, rc);
    return 0;
}

int uaes_poly1305_batch(int keybits, const uint8_t *keys, const uint8_t *nonces, size_t nmsg,
                        size_t msg_bytes, const void *data, uint8_t *macs)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_nonces = NULL;
    int rc;
    if (msg_bytes && nmsg > (size_t)-1 / msg_bytes) return fail(UAES_E_ARG, "batch size overflows");
    if (!keys || (nmsg && (!nonces || !macs)) || (nmsg && msg_bytes && !data)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&ks, keys, keybits)) != 0) return rc;
    if (nmsg == 0) { burn(&ks, sizeof ks); return 0; }
    if ((rc = enter(&c, &L)) != 0) { burn(&ks, sizeof ks); return rc; }
    do {
        if ((rc = stage_aad(L, nonces, nmsg * 16, &d_nonces)) != 0) break;       /* host nonces -> device */
        if ((rc = plan_io(L, data, nmsg * msg_bytes, macs, nmsg * 16, &io)) != 0) break;
        if (io.dout == io.din && io.copy_back) {                  /* MACs must not overwrite unread messages */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], nmsg * 16 + 64)) { rc = UAES_E_HIP; break; }
            io.dout = L->stage[1];
        }
        int k = uaesk_poly1305_batch(L->stream, &c->tb, ks.nr, &ks.ek, keys + keybits / 8, d_nonces, nmsg, msg_bytes,
                                     io.din, io.dout);
        if (k) { rc = fail(UAES_E_HIP, "poly1305 batch launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, nmsg * 16);
    } while (0);
    burn(&ks, sizeof ks);
    DONE(L, rc);
}

static int ccm_lens_ok(size_t nonceLen, size_t tagLen)
{
    if (nonceLen < 7 || nonceLen > 13) return fail(UAES_E_ARG, "CCM nonce length %zu (7..13)", nonceLen);
    if (tagLen < 4 || tagLen > 16 || (tagLen & 1)) return fail(UAES_E_ARG, "CCM tag length %zu (even, 4..16)", tagLen);
    return 0;
}

/* nonceLen / tagLen = the reference's compile-time CCM_NONCE_LEN / CCM_TAG_LEN (micro_aes.h:103-104) */
int uaes_ccm_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_aad;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = ccm_lens_ok(nonceLen, tagLen)) != 0) return rc;
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(pntxt, crtxt, ptextLen, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&ks);
        HOST_RET(ks, uaesh_ccm(&hk, 0, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)pntxt, ptextLen, (uint8_t *)crtxt));
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, pntxt, ptextLen, crtxt, ptextLen + tagLen, &io)) != 0) break;
        int k = uaesk_ccm(L->stream, &c->tb, ks.nr, &ks.ek, 0, nonce, nonceLen, tagLen, d_aad, aDataLen,
                          io.din, ptextLen, io.dout, NULL);
        if (k) { rc = fail(UAES_E_HIP, "ccm launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, ptextLen + tagLen);
    } while (0);
    DONE(L, rc);
}

int uaes_ccm_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, void *crtxt)
{
    return uaes_ccm_encrypt_ex(keybits, key, nonce, 11, 16, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_ccm_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_aad;
    int rc, status = -1;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !crtxt || (crtxtLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = ccm_lens_ok(nonceLen, tagLen)) != 0) return rc;
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(crtxt, pntxt, crtxtLen, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&ks);
        rc = uaesh_ccm(&hk, 1, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)crtxt, crtxtLen, (uint8_t *)pntxt);
        if (rc && wipe_on_auth_failure()) memset(pntxt, 0, crtxtLen);       /* (the default leaves the text, as the reference does) */
        HOST_RET(ks, rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, crtxt, crtxtLen + tagLen, pntxt, crtxtLen, &io)) != 0) break;
        int k = uaesk_ccm(L->stream, &c->tb, ks.nr, &ks.ek, 1, nonce, nonceLen, tagLen, d_aad, aDataLen,
                          io.din, crtxtLen, io.dout, L->d_status);
        if (k) { rc = fail(UAES_E_HIP, "ccm launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) break;
        io.drained = 1;                              /* (a second wait costs another ticket kernel) */
        /* the reference decrypts before it authenticates and (SABOTAGE being a
         * no-op in its default build) leaves the text in place on a mismatch   */
        if ((rc = status ? finish_io_unauthenticated(&io, crtxtLen) : finish_io(&io, crtxtLen)) != 0) break;
        rc = status ? UAES_E_AUTHENTICATION : 0;
    } while (0);
    DONE(L, rc);
}

int uaes_ccm_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return uaes_ccm_decrypt_ex(keybits, key, nonce, 11, 16, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

/* ------------------------------------------------------------------------ */
/* EAX and SIV, RFC 5297 (AES_EAX_* micro_aes.c:1560-1648, AES_SIV_* :1373-1411) */
/* ------------------------------------------------------------------------ */
/* Kernels in uaes_eax_siv.hip.  A text of at most UAES_EAX_SIV_SMALL_MAX bytes is one launch; a longer one runs its
 * independent chains in one launch, reads the counter block (and the verdict) back in one fetch and hands it to the
 * positioned CTR kernels.  Side arrays (nonce, AAD) in host memory travel through the lane's scratch.             */
#define SIDE(n) (((n) + 15) & ~(size_t)15)

static int side_in(lane *L, size_t *off, const void *src, size_t n, const void **d)
{
    *d = NULL;
    if (!n) return 0;
    if (is_device_ptr(src)) { *d = src; return wait_for_callers_device_work(); }
    *d = (char *)L->scratch + *off;
    *off += SIDE(n);
    HIPCHK(hipMemcpyAsync((void *)*d, src, n, hipMemcpyHostToDevice, (hipStream_t)L->stream));
    return 0;
}

/* 16 bytes (an IV) from host or device memory to host memory, or back */
static int iv_read(uint8_t out[16], const uint8_t *iv)
{
    if (is_device_ptr(iv)) { HIPCHK(hipMemcpy(out, iv, 16, hipMemcpyDeviceToHost)); }
    else memcpy(out, iv, 16);
    return 0;
}
static int iv_write(uint8_t *iv, const uint8_t v[16])
{
    if (is_device_ptr(iv)) { HIPCHK(hipMemcpy(iv, v, 16, hipMemcpyHostToDevice)); }
    else memcpy(iv, v, 16);
    return 0;
}

#define HIPCHK_GOTO(call)                                                                            \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) { rc = fail(UAES_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); goto out; } \
    } while (0)
#define ES_KCHK(what, call)                                                                           \
    do {                                                                                              \
        const int k_ = (call);                                                                        \
        if (k_) { rc = fail(UAES_E_HIP, what " launch: %s", hipGetErrorString((hipError_t)k_)); goto out; } \
    } while (0)

static int eax_common(int keybits, const uint8_t *key, int decrypt, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                      const void *aData, size_t aDataLen, const void *in, size_t len, void *outp)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_nonce, *d_aad;
    size_t off = 0;
    int rc, status = 0;
    uint8_t res[32];
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!in || (len && !outp) || (nonceLen && !nonce)) return fail(UAES_E_ARG, "NULL pointer");
    if (!decrypt && !outp) return fail(UAES_E_ARG, "NULL pointer");
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "EAX tag length %zu (1..16)", tagLen);
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(in, outp, len, 1) && !is_device_ptr(aData) && !is_device_ptr(nonce)) {
        const uaesh_key hk = host_key(&ks);
        HOST_RET(ks, uaesh_eax(&hk, decrypt, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen,
                               (const uint8_t *)in, len, (uint8_t *)outp));
    }
    if ((rc = enter(&c, &L)) != 0) { burn(&ks, sizeof ks); return rc; }
    if ((rc = lane_scratch(L, SIDE(nonceLen) + SIDE(aDataLen), SCRATCH_OTHER)) != 0) goto out;
    if ((rc = side_in(L, &off, nonce, nonceLen, &d_nonce)) != 0) goto out;
    if ((rc = side_in(L, &off, aData, aDataLen, &d_aad)) != 0) goto out;
    if (decrypt) rc = plan_io(L, in, len + tagLen, outp, len, &io);
    else rc = plan_io(L, in, len, outp, len + tagLen, &io);
    if (rc) goto out;
    {
        unsigned char *tag = decrypt ? (unsigned char *)io.din + len : (unsigned char *)io.dout + len;
        const unsigned tl = (unsigned)tagLen;
        if (len <= UAES_EAX_SIV_SMALL_MAX) {             /* eax.small: one launch */
            ES_KCHK("eax", uaesk_eax_small(L->stream, &c->tb, ks.nr, &ks.ek, decrypt, d_nonce, nonceLen, d_aad, aDataLen,
                                           io.din, len, io.dout, tag, tl, decrypt ? L->d_status : NULL));
            if (decrypt) {
                if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) goto out;
                io.drained = 1;
            }
        } else {                                          /* eax.long: the chains, one fetch, then CTR */
            uaesk_ctr ctr;
            ES_KCHK("eax", uaesk_eax_macs(L->stream, &c->tb, ks.nr, &ks.ek, decrypt ? 1 : 0, d_nonce, nonceLen,
                                          d_aad, aDataLen, decrypt ? io.din : NULL, decrypt ? len : 0, tag, tl, L->d_status));
            if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
            memcpy(&status, res, sizeof status);
            if (decrypt && status) {
                io.drained = 1;
            } else {
                make_ctr(&ctr, res + 16, 0);
                ES_KCHK("eax ctr", uaesk_ctr_xcrypt(L->stream, &c->tb, ks.nr, &ks.ek, &ctr, io.din, io.dout, len, NULL));
                if (!decrypt)
                    ES_KCHK("eax", uaesk_eax_macs(L->stream, &c->tb, ks.nr, &ks.ek, 2, NULL, 0, NULL, 0, io.dout, len,
                                                  tag, tl, L->d_status));
            }
        }
    }
    /* the tag is checked before anything is written (:1638-1645): a forgery leaves pntxt as it was */
    if (decrypt && status) rc = UAES_E_AUTHENTICATION;
    else rc = finish_io(&io, decrypt ? len : len + tagLen);
out:
    burn(&ks, sizeof ks);
    memset(res, 0, sizeof res);
    DONE(L, rc);
}

int uaes_eax_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                     const void *aData, size_t aDataLen, const void *pntxt, size_t ptextLen, void *crtxt)
{
    if (!pntxt && !ptextLen) pntxt = crtxt;                       /* (nothing is read) */
    return eax_common(keybits, key, 0, nonce, nonceLen, tagLen, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_eax_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                     const void *aData, size_t aDataLen, const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return eax_common(keybits, key, 1, nonce, nonceLen, tagLen, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

static int siv_keys(keysched *k1, keysched *k2, const uint8_t *keys, int keybits)
{
    int rc;
    if (!keys) return fail(UAES_E_ARG, "NULL keys");
    if ((rc = expand_key(k1, keys, keybits)) != 0) return rc;
    return expand_key(k2, keys + keybits / 8, keybits);
}

static int siv_common(int keybits, const uint8_t *keys, int decrypt, uint8_t *iv, const void *aData, size_t aDataLen,
                      const void *in, size_t len, void *outp)
{
    context *c;
    lane *L;
    keysched k1, k2;
    io_plan io;
    const void *d_aad;
    size_t off = 0;
    int rc, status = 0;
    uint8_t v[16], res[32];
    if ((rc = siv_keys(&k1, &k2, keys, keybits)) != 0) return rc;
    if (!iv || (len && (!in || !outp))) return fail(UAES_E_ARG, "NULL pointer");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (decrypt && (rc = iv_read(v, iv)) != 0) return rc;
    if (host_take(in, outp, len, 1) && !is_device_ptr(aData) && !is_device_ptr(iv)) {
        const uaesh_key h1 = host_key(&k1), h2 = host_key(&k2);
        rc = uaesh_siv(&h1, &h2, decrypt, v, (const uint8_t *)aData, aDataLen, (const uint8_t *)in, len, (uint8_t *)outp);
        burn(&k1, sizeof k1);
        burn(&k2, sizeof k2);
        if (!decrypt) memcpy(iv, v, 16);
        if (rc && len && wipe_on_auth_failure()) memset(outp, 0, len);       /* (the default leaves the text, as the reference does) */
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) { burn(&k1, sizeof k1); burn(&k2, sizeof k2); return rc; }
    if ((rc = lane_scratch(L, SIDE(aDataLen), SCRATCH_OTHER)) != 0) goto out;
    if ((rc = side_in(L, &off, aData, aDataLen, &d_aad)) != 0) goto out;
    if ((rc = plan_io(L, len ? in : NULL, len, len ? outp : NULL, len, &io)) != 0) goto out;
    if (len <= UAES_EAX_SIV_SMALL_MAX) {                  /* s2v.small: one launch */
        ES_KCHK("siv", uaesk_s2v_small(L->stream, &c->tb, k1.nr, &k1.ek, &k2.ek, decrypt, decrypt ? v : NULL, d_aad,
                                       aDataLen, io.din, len, io.dout, (char *)L->d_status + 16,
                                       decrypt ? L->d_status : NULL));
        if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
        io.drained = 1;
    } else if (!decrypt) {                                /* s2v.long: the chains, one fetch, then CTR(V') */
        uaesk_ctr ctr;
        ES_KCHK("siv", uaesk_s2v_macs(L->stream, &c->tb, k1.nr, &k1.ek, 0, NULL, d_aad, aDataLen, io.din, len, L->d_status));
        if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
        memcpy(v, res + 16, 16);
        v[8] &= 0x7F;
        v[12] &= 0x7F;
        make_ctr(&ctr, v, 0);
        ES_KCHK("siv ctr", uaesk_ctr_xcrypt(L->stream, &c->tb, k2.nr, &k2.ek, &ctr, io.din, io.dout, len, NULL));
    } else {                                              /* decrypt: CTR(iv') first, S2V over what it wrote, one fetch */
        uaesk_ctr ctr;
        uint8_t cv[16];
        memcpy(cv, v, 16);
        cv[8] &= 0x7F;
        cv[12] &= 0x7F;
        make_ctr(&ctr, cv, 0);
        ES_KCHK("siv ctr", uaesk_ctr_xcrypt(L->stream, &c->tb, k2.nr, &k2.ek, &ctr, io.din, io.dout, len, NULL));
        ES_KCHK("siv", uaesk_s2v_macs(L->stream, &c->tb, k1.nr, &k1.ek, 1, v, d_aad, aDataLen, io.dout, len, L->d_status));
        if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
        io.drained = 1;
    }
    if (decrypt) {
        memcpy(&status, res, sizeof status);
        /* like the reference: the text is written before it is authenticated; SABOTAGE = uaes_set_wipe_on_auth_failure */
        if ((rc = status ? finish_io_unauthenticated(&io, len) : finish_io(&io, len)) == 0 && status) rc = UAES_E_AUTHENTICATION;
    } else {
        memcpy(v, res + 16, 16);
        if ((rc = finish_io(&io, len)) == 0) rc = iv_write(iv, v);
    }
out:
    burn(&k1, sizeof k1);
    burn(&k2, sizeof k2);
    DONE(L, rc);
}

int uaes_siv_encrypt(int keybits, const uint8_t *keys, const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, uint8_t iv[16], void *crtxt)
{
    return siv_common(keybits, keys, 0, iv, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_siv_decrypt(int keybits, const uint8_t *keys, const uint8_t iv[16], const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return siv_common(keybits, keys, 1, (uint8_t *)iv, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

/* Batches: nmsg records of msg_bytes each under one key, sixteen lanes per record.  Every array may be host or
 * device memory; host arrays travel through the lane's staging buffers and scratch.  An EAX decryption writes only
 * authentic records: the output buffer starts as the caller's (host memory is copied in first).                   */
static int stage_text(lane *L, int k, const void *user, size_t n, int prefill, void **d)
{
    if (!n) { *d = NULL; return 0; }
    if (is_device_ptr(user)) { *d = (void *)user; return wait_for_callers_device_work(); }
    if (grow_on(L->stream, &L->stage[k], &L->stage_cap[k], n + 64)) return UAES_E_HIP;
    *d = L->stage[k];
    if (prefill) HIPCHK(hipMemcpyAsync(*d, user, n, hipMemcpyHostToDevice, (hipStream_t)L->stream));
    return 0;
}

static int side_out(lane *L, size_t *off, void *user, size_t n, void **d)
{
    if (is_device_ptr(user)) { *d = user; return 0; }
    *d = (char *)L->scratch + *off;
    *off += SIDE(n);
    return 0;
}

static int copy_out(lane *L, void *user, const void *d, size_t n)
{
    if (!n || d == user) return 0;
    HIPCHK(hipMemcpyAsync(user, d, n, hipMemcpyDeviceToHost, (hipStream_t)L->stream));
    return 0;
}

static int aead_batch(int siv, int decrypt, int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                      const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                      const void *in, void *outp, uint8_t *tags, uint8_t *verdicts)
{
    context *c;
    lane *L;
    keysched k1, k2;
    const void *d_nonces = NULL, *d_aad = NULL, *d_tags_in = NULL;
    void *d_in = NULL, *d_out = NULL, *d_tags = NULL, *d_verdicts = NULL;
    size_t off = 0;
    int rc, bad = 0;
    if ((msg_bytes && nmsg > (size_t)-1 / msg_bytes) || (nonce_len && nmsg > (size_t)-1 / nonce_len) ||
        (aad_bytes && nmsg > (size_t)-1 / aad_bytes) || nmsg > (size_t)-1 / 16)
        return fail(UAES_E_ARG, "batch size overflows");
    if ((rc = siv ? siv_keys(&k1, &k2, key, keybits) : expand_key(&k1, key, keybits)) != 0) return rc;
    if (nmsg == 0) { burn(&k1, sizeof k1); burn(&k2, sizeof k2); return 0; }
    {
        const size_t total = nmsg * msg_bytes;
        if ((total && (!in || !outp)) || !tags || (decrypt && !verdicts) || (!siv && nonce_len && !nonces) ||
            (aad_bytes && !aData)) {
            burn(&k1, sizeof k1); burn(&k2, sizeof k2);
            return fail(UAES_E_ARG, "NULL pointer");
        }
        if ((rc = enter(&c, &L)) != 0) { burn(&k1, sizeof k1); burn(&k2, sizeof k2); return rc; }
        if ((rc = lane_scratch(L, SIDE(nmsg * nonce_len) + SIDE(nmsg * aad_bytes) + SIDE(nmsg * 16) + SIDE(nmsg),
                               SCRATCH_OTHER)) != 0) goto out;
        if (!siv && (rc = side_in(L, &off, nonces, nmsg * nonce_len, &d_nonces)) != 0) goto out;
        if ((rc = side_in(L, &off, aData, nmsg * aad_bytes, &d_aad)) != 0) goto out;
        if (decrypt) {
            if ((rc = side_in(L, &off, tags, nmsg * 16, &d_tags_in)) != 0) goto out;
            d_tags = (void *)d_tags_in;
            if ((rc = side_out(L, &off, verdicts, nmsg, &d_verdicts)) != 0) goto out;
        } else if ((rc = side_out(L, &off, tags, nmsg * 16, &d_tags)) != 0) goto out;
        if ((rc = stage_text(L, 0, in, total, 1, &d_in)) != 0) goto out;
        if ((rc = stage_text(L, 1, outp, total, decrypt && !siv, &d_out)) != 0) goto out;
        if (decrypt) HIPCHK_GOTO(hipMemsetAsync(L->d_status, 0, sizeof(int), (hipStream_t)L->stream));
        if (siv)
            ES_KCHK("siv batch", uaesk_s2v_batch(L->stream, &c->tb, k1.nr, &k1.ek, &k2.ek, decrypt, wipe_on_auth_failure(),
                                                 d_aad, aad_bytes, nmsg, msg_bytes, d_in, d_out, d_tags, d_verdicts,
                                                 L->d_status));
        else
            ES_KCHK("eax batch", uaesk_eax_batch(L->stream, &c->tb, k1.nr, &k1.ek, decrypt, d_nonces, nonce_len, d_aad,
                                                 aad_bytes, nmsg, msg_bytes, d_in, d_out, d_tags, d_verdicts, L->d_status));
        if ((rc = copy_out(L, outp, d_out, total)) != 0) goto out;
        if ((rc = decrypt ? copy_out(L, verdicts, d_verdicts, nmsg) : copy_out(L, tags, d_tags, nmsg * 16)) != 0) goto out;
        if (decrypt) HIPCHK_GOTO(hipMemcpyAsync(&bad, L->d_status, sizeof bad, hipMemcpyDeviceToHost, (hipStream_t)L->stream));
        HIPCHK_GOTO(hipStreamSynchronize((hipStream_t)L->stream));
        rc = bad ? UAES_E_AUTHENTICATION : 0;
    }
out:
    burn(&k1, sizeof k1);
    burn(&k2, sizeof k2);
    DONE(L, rc);
}

int uaes_eax_encrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                           const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags)
{
    return aead_batch(0, 0, keybits, key, nmsg, msg_bytes, nonces, nonce_len, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_eax_decrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                           const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return aead_batch(0, 1, keybits, key, nmsg, msg_bytes, nonces, nonce_len, aData, aad_bytes, crtxt, pntxt,
                      (uint8_t *)tags, verdicts);
}

int uaes_siv_encrypt_batch(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes,
                           const void *aData, size_t aad_bytes, const void *pntxt, uint8_t *ivs, void *crtxt)
{
    return aead_batch(1, 0, keybits, keys, nmsg, msg_bytes, NULL, 0, aData, aad_bytes, pntxt, crtxt, ivs, NULL);
}

int uaes_siv_decrypt_batch(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes,
                           const void *aData, size_t aad_bytes, const uint8_t *ivs, const void *crtxt, void *pntxt,
                           uint8_t *verdicts)
{
    return aead_batch(1, 1, keybits, keys, nmsg, msg_bytes, NULL, 0, aData, aad_bytes, crtxt, pntxt, (uint8_t *)ivs,
                      verdicts);
}

/* ------------------------------------------------------------------------ */
/* CBC / CFB / OFB                                   */
/* ------------------------------------------------------------------------ */
/* mode: 0 CBC enc, 1 CBC dec, 2 CFB enc, 3 CFB dec, 4 OFB; the CBC of a reference build with CTS 0 (micro_aes.h:56):
 * 5 + p CBC enc that pads its last chunk with AES_PADDING p (micro_aes.c:727-733), 8 CBC dec of whole blocks (:761) */
static int feedback_common(int keybits, const uint8_t *key, const uint8_t *iVec, int mode,
                           const void *in, size_t len, void *out)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    int rc;
    size_t out_len = len;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!iVec) return fail(UAES_E_ARG, "NULL iVec");
    if (mode <= 1 && len < 16) return UAES_E_DATALENGTH;          /* CTS: data size >= BLOCKSIZE (:708, :758) */
    if (mode == 8 && len % 16) return UAES_E_DATALENGTH;          /* no CTS: whole blocks (:761)              */
    if (mode >= 5 && mode <= 7) {
        if (len > (size_t)-1 - 16) return fail(UAES_E_ARG, "length overflows");
        out_len = len - len % 16 + ((len % 16 || mode > 5) ? 16 : 0);       /* padBlock (:610-621)            */
    }
    if (out_len == 0) return 0;
    if ((len && !in) || !out) return fail(UAES_E_ARG, "NULL data pointer");
    /* the encrypting directions and OFB are ONE serial chain; the decrypting directions of CBC and CFB are block-parallel */
    if (host_take(in, out, len, !(mode == 1 || mode == 3 || mode == 8))) {
        const uaesh_key hk = host_key(&ks);
        const uint8_t *x = (const uint8_t *)in;
        uint8_t *y = (uint8_t *)out;
        switch (mode) {
        case 0: HOST_RET(ks, uaesh_cbc_encrypt(&hk, iVec, 1, 0, x, len, y));
        case 1: HOST_RET(ks, uaesh_cbc_decrypt(&hk, iVec, 1, x, len, y));
        case 2: uaesh_cfb(&hk, iVec, 1, x, len, y); HOST_RET(ks, 0);
        case 3: uaesh_cfb(&hk, iVec, 0, x, len, y); HOST_RET(ks, 0);
        case 4: uaesh_ofb(&hk, iVec, x, len, y); HOST_RET(ks, 0);
        case 8: HOST_RET(ks, uaesh_cbc_decrypt(&hk, iVec, 0, x, len, y));
        default: HOST_RET(ks, uaesh_cbc_encrypt(&hk, iVec, 0, mode - 5, x, len, y));
        }
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = plan_io(L, in, len, out, out_len, &io)) != 0) break;
        if ((mode == 1 || mode == 3 || mode == 8) && io.din == io.dout) {
            /* the parallel directions read C_{i-1} from the input: give them a private copy */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], len + 64)) { rc = UAES_E_HIP; break; }
            if (hipMemcpyAsync(L->stage[1], io.din, len, hipMemcpyDeviceToDevice, (hipStream_t)L->stream) != hipSuccess) {
                rc = fail(UAES_E_HIP, "input copy failed");
                break;
            }
            io.din = L->stage[1];
        }
        int k = uaesk_feedback(L->stream, &c->tb, ks.nr, &ks.ek, &ks.dk, mode, iVec, io.din, len, io.dout);
        if (k) { rc = fail(UAES_E_HIP, "feedback-mode launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, out_len);
    } while (0);
    DONE(L, rc);
}

/* CBC as a reference build with CTS 0 does it (micro_aes.h:56, micro_aes.c:704-733, :753-761): no ciphertext stealing
 * and no minimum length; the last chunk is padded like ECB's (padding = AES_PADDING: 0 zeros behind a partial chunk,
 * 1 PKCS#7 / 2 ISO 7816-4 always append), so crtxt receives 16 * (ptextLen / 16 + (ptextLen % 16 || padding)) bytes;
 * decryption wants whole blocks (else UAES_E_DATALENGTH) and leaves the padding in place                         */
int uaes_cbc_encrypt_padded(int keybits, const uint8_t *key, const uint8_t *iVec, int padding,
                            const void *pntxt, size_t ptextLen, void *crtxt)
{
    if (padding < 0 || padding > 2) return fail(UAES_E_ARG, "padding %d (0 zeros, 1 PKCS#7, 2 ISO/IEC 7816-4)", padding);
    return feedback_common(keybits, key, iVec, 5 + padding, pntxt, ptextLen, crtxt);
}

int uaes_cbc_decrypt_blocks(int keybits, const uint8_t *key, const uint8_t *iVec,
                            const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return feedback_common(keybits, key, iVec, 8, crtxt, crtxtLen, pntxt);
}

int uaes_cbc_encrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *pntxt, size_t ptextLen, void *crtxt)
{
    return feedback_common(keybits, key, iVec, 0, pntxt, ptextLen, crtxt);
}

int uaes_cbc_decrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return feedback_common(keybits, key, iVec, 1, crtxt, crtxtLen, pntxt);
}

int uaes_cfb_encrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *pntxt, size_t ptextLen, void *crtxt)
{
    return feedback_common(keybits, key, iVec, 2, pntxt, ptextLen, crtxt);
}

int uaes_cfb_decrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return feedback_common(keybits, key, iVec, 3, crtxt, crtxtLen, pntxt);
}

int uaes_ofb_xcrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                    const void *in, size_t len, void *out)
{
    return feedback_common(keybits, key, iVec, 4, in, len, out);
}

/* ------------------------------------------------------------------------ */
/* batches of independent chains (one GPU lane per message)                     */
/* ------------------------------------------------------------------------ */
static int batch_common(int keybits, const uint8_t *key, int mac, const uint8_t *ivs, size_t nmsg,
                        size_t msg_bytes, const void *in, void *out)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_ivs = NULL;
    int rc;
    const size_t total = nmsg * msg_bytes, out_len = mac ? nmsg * 16 : total;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!mac && (msg_bytes < 16 || msg_bytes % 16))
        return fail(UAES_E_ARG, "batched CBC: every message must be a whole number of blocks (got %zu bytes)", msg_bytes);
    if (msg_bytes && nmsg > (size_t)-1 / msg_bytes) return fail(UAES_E_ARG, "batch size overflows");
    if (nmsg == 0) return 0;
    if ((total && !in) || !out || (!mac && !ivs)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if (!mac && (rc = stage_aad(L, ivs, nmsg * 16, &d_ivs)) != 0) break;     /* host IVs -> device */
        if (!mac && (((uintptr_t)d_ivs) & 15u)) { rc = fail(UAES_E_ARG, "device IV array must be 16-byte aligned"); break; }
        if ((rc = plan_io(L, in, total, out, out_len, &io)) != 0) break;
        if (mac && io.dout == io.din && io.copy_back) {          /* MACs must not overwrite unread messages */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], out_len + 64)) { rc = UAES_E_HIP; break; }
            io.dout = L->stage[1];
        }
        int k = uaesk_chain_batch(L->stream, &c->tb, ks.nr, &ks.ek, mac, d_ivs, nmsg, msg_bytes, io.din, io.dout);
        if (k) { rc = fail(UAES_E_HIP, "batch launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, out_len);
    } while (0);
    DONE(L, rc);
}

int uaes_cbc_encrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const void *pntxt, void *crtxt)
{
    return batch_common(keybits, key, 0, ivs, nmsg, msg_bytes, pntxt, crtxt);
}

int uaes_cmac_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                    const void *data, uint8_t *macs)
{
    return batch_common(keybits, key, 1, NULL, nmsg, msg_bytes, data, macs);
}

/* ------------------------------------------------------------------------ */
/* GCM-SIV (RFC 8452; micro_aes.c:1418-1516)          */
/* ------------------------------------------------------------------------ */
/* Host orchestration only: the host expands the MASTER key and enqueues; key derivation, the derived key's
 * expansion, POLYVAL, the tag and the LE32 counter stream run in kernels and their per-nonce values never leave the
 * device (k_siv_small for a short message, uaesk_gcmsiv_long otherwise).                                       */
int uaes_gcmsiv_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    context *c;
    lane *L;
    io_plan io;
    const void *d_aad;
    int rc;
    if (keybits != 128 && keybits != 192 && keybits != 256)
        return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if (!key || !nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(pntxt, crtxt, ptextLen, 0) && !is_device_ptr(aData)) {
        keysched mk;
        uaesh_key hk;
        if ((rc = expand_key(&mk, key, keybits)) != 0) return rc;
        hk = host_key(&mk);
        rc = uaesh_gcmsiv(&hk, keybits, 0, nonce, (const uint8_t *)aData, aDataLen, (const uint8_t *)pntxt, ptextLen, (uint8_t *)crtxt, uaes_expand_key);
        burn(&mk, sizeof mk);
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = gcm_scratch(L, SCRATCH_OTHER)) != 0) break;
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, pntxt, ptextLen, crtxt, ptextLen + 16, &io)) != 0) break;
        {   /* a short message is ONE launch (k_siv_small): key derivation, POLYVAL, tag and keystream in one
             * workgroup; the host only expands the master key */
            keysched master;
            if ((rc = expand_key(&master, key, keybits)) != 0) break;
            int ks = uaesk_gcmsiv_small(L->stream, &c->tb, master.nr, &master.ek, 0, nonce, d_aad, aDataLen,
                                        io.din, ptextLen, io.dout, NULL);
            memset(&master, 0, sizeof master);
            if (ks > 0) { rc = fail(UAES_E_HIP, "gcm-siv launch: %s", hipGetErrorString((hipError_t)ks)); break; }
            if (ks == 0) { rc = finish_io(&io, ptextLen + 16); break; }
        }
        {   /* a longer one: six or seven launches one behind the other, the per-nonce key, the hash, the tag and the
             * counter made of it stay on the device (uaesk_gcmsiv_long) -- the host waits once, in finish_io */
            keysched master;
            if ((rc = expand_key(&master, key, keybits)) != 0) break;
            arm_done_word(scratch_done_word(L->scratch, L->scratch_cap));
            int kl = uaesk_gcmsiv_long(L->stream, &c->tb, master.nr, &master.ek, 0, nonce, d_aad, aDataLen,
                                       io.din, ptextLen, io.dout, L->scratch, NULL);
            arm_done_word(NULL);
            memset(&master, 0, sizeof master);
            if (kl) { rc = fail(UAES_E_HIP, "gcm-siv launch: %s", hipGetErrorString((hipError_t)kl)); break; }
        }
        rc = finish_io(&io, ptextLen + 16);
    } while (0);
    DONE(L, rc);
}

int uaes_gcmsiv_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    io_plan io;
    const void *d_aad;
    int rc;
    if (keybits != 128 && keybits != 192 && keybits != 256)
        return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if (!key || !nonce || !crtxt || (crtxtLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(crtxt, pntxt, crtxtLen, 0) && !is_device_ptr(aData)) {
        keysched mk;
        uaesh_key hk;
        if ((rc = expand_key(&mk, key, keybits)) != 0) return rc;
        hk = host_key(&mk);
        rc = uaesh_gcmsiv(&hk, keybits, 1, nonce, (const uint8_t *)aData, aDataLen, (const uint8_t *)crtxt, crtxtLen, (uint8_t *)pntxt, uaes_expand_key);
        burn(&mk, sizeof mk);
        if (rc == UAES_E_AUTHENTICATION && wipe_on_auth_failure()) memset(pntxt, 0, crtxtLen);
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = gcm_scratch(L, SCRATCH_OTHER)) != 0) break;
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, crtxt, crtxtLen + 16, pntxt, crtxtLen, &io)) != 0) break;
        {   /* a short message is ONE launch (k_siv_small), key derivation included */
            keysched master;
            if ((rc = expand_key(&master, key, keybits)) != 0) break;
            int ks = uaesk_gcmsiv_small(L->stream, &c->tb, master.nr, &master.ek, 1, nonce, d_aad, aDataLen,
                                        io.din, crtxtLen, io.dout, L->d_status);
            memset(&master, 0, sizeof master);
            if (ks > 0) { rc = fail(UAES_E_HIP, "gcm-siv launch: %s", hipGetErrorString((hipError_t)ks)); break; }
            if (ks == 0) {
                int status = -1;
                if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) break;
                io.drained = 1;
                if ((rc = status ? finish_io_unauthenticated(&io, crtxtLen) : finish_io(&io, crtxtLen)) != 0) break;
                rc = status ? UAES_E_AUTHENTICATION : 0;
                break;
            }
        }
        {   /* like the reference: decrypt with the RECEIVED tag as counter, then authenticate (:1500-1502) -- all of
             * it on the device (uaesk_gcmsiv_long); the text stays (SABOTAGE is a no-op) unless
             * uaes_set_wipe_on_auth_failure(1) */
            keysched master;
            int status = -1;
            if ((rc = expand_key(&master, key, keybits)) != 0) break;
            arm_done_word(scratch_done_word(L->scratch, L->scratch_cap));
            int kl = uaesk_gcmsiv_long(L->stream, &c->tb, master.nr, &master.ek, 1, nonce, d_aad, aDataLen,
                                       io.din, crtxtLen, io.dout, L->scratch, L->d_status);
            arm_done_word(NULL);
            memset(&master, 0, sizeof master);
            if (kl) { rc = fail(UAES_E_HIP, "gcm-siv launch: %s", hipGetErrorString((hipError_t)kl)); break; }
            if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) break;
            io.drained = 1;
            if ((rc = status ? finish_io_unauthenticated(&io, crtxtLen) : finish_io(&io, crtxtLen)) != 0) break;
            rc = status ? UAES_E_AUTHENTICATION : 0;
        }
    } while (0);
    DONE(L, rc);
}

/* ------------------------------------------------------------------------ */
/* OCB (RFC 7253; AES_OCB_encrypt / AES_OCB_decrypt, micro_aes.c:1774-1811)     */
/* ------------------------------------------------------------------------ */
/* nonceLen / tagLen = the reference's compile-time OCB_NONCE_LEN (1..15) / OCB_TAG_LEN (1..16), micro_aes.h:115-116 */
static int ocb_common(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen, int decrypt,
                      const void *aData, size_t aDataLen, const void *in, size_t len, void *out)
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_aad;
    int rc, status = -1;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || (!decrypt && !out) || (len && (!in || !out)) || (decrypt && !in))
        return fail(UAES_E_ARG, "NULL pointer");
    if (nonceLen < 1 || nonceLen > 15) return fail(UAES_E_ARG, "OCB nonce length %zu (1..15)", nonceLen);
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "OCB tag length %zu (1..16)", tagLen);
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(in, out, len, 0) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&ks);
        rc = uaesh_ocb(&hk, decrypt, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)in, len, (uint8_t *)out);
        if (rc < 0) return fail(UAES_E_HIP, "out of host memory");
        if (rc == UAES_E_AUTHENTICATION && wipe_on_auth_failure()) memset(out, 0, len);
        HOST_RET(ks, rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = gcm_scratch(L, SCRATCH_OTHER)) != 0) break;        /* >= uaesk_ocb_scratch_bytes() */
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, in, len + (decrypt ? tagLen : 0), out, len + (decrypt ? 0 : tagLen), &io)) != 0) break;
        int *st_where = lane_status(L);
        if (!decrypt || st_where != L->d_status) {            /* a one-launch call may carry the completion ticket */
            if (decrypt) *(volatile int *)st_where = -1;
            ticket_arm(L, len);
        }
        int k = uaesk_ocb(L->stream, &c->tb, ks.nr, &ks.ek, &ks.dk, decrypt, nonce, nonceLen, tagLen, d_aad, aDataLen,
                          io.din, len, io.dout, L->scratch, scratch_done_word(L->scratch, L->scratch_cap), st_where);
        ticket_armed_launch_done(L);
        if (k) { rc = fail(UAES_E_HIP, "ocb launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if (decrypt) {
            if ((rc = lane_read_status(L, st_where, &status)) != 0) break;
            io.drained = 1;
        }
        /* decrypt: the text stays on a bad tag, as in the reference, unless wiping is switched on */
        if ((rc = (decrypt && status != 0) ? finish_io_unauthenticated(&io, len)
                                           : finish_io(&io, len + (decrypt ? 0 : tagLen))) != 0) break;
        if (decrypt && status != 0) rc = UAES_E_AUTHENTICATION;
    } while (0);
    DONE(L, rc);
}

int uaes_ocb_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, void *crtxt)
{
    return ocb_common(keybits, key, nonce, 12, 16, 0, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_ocb_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    return ocb_common(keybits, key, nonce, nonceLen, tagLen, 0, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_ocb_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return ocb_common(keybits, key, nonce, nonceLen, tagLen, 1, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

int uaes_ocb_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return ocb_common(keybits, key, nonce, 12, 16, 1, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

int uaes_ocb_dev(int keybits, const uint8_t *key, const uint8_t *nonce, int decrypt,
                 const void *d_aad, size_t aad_len,
                 const void *d_in, size_t len, void *d_out, int *d_status, void *stream)
{
    context *c;
    keysched ks;
    void *scr;
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || (decrypt ? !d_in : !d_out)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if (decrypt && !d_status) return fail(UAES_E_ARG, "NULL d_status");
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    KCHK_PINNED(c, slot, uaesk_ocb(stream, &c->tb, ks.nr, &ks.ek, &ks.dk, decrypt, nonce, 12, 16, d_aad, aad_len, d_in, len,
                                   d_out, scr, scratch_done_word(scr, c->slot[slot].cap), d_status));
    return 0;
}

/* ------------------------------------------------------------------------ */
/* streamed GCM: begin / update ... / finish                  */
/* ------------------------------------------------------------------------ */
struct uaes_gcm_stream {
    keysched  ks;
    uint8_t   nonce[12];
    int       decrypt, closed, device;
    uint64_t  aad_len, done;        /* bytes of text absorbed so far */
    unsigned  plan_state;           /* which GHASH tables the scratch holds (uaesk_gcm_stream_absorb) */
    void     *scratch;              /* uaesk_gcm_stream_scratch_bytes() + 64: tables, running GHASH, tag, status */
};

/* (the whole GCM layout: a long piece takes the one-pass kernel, which needs its tables there) */
#define STREAM_SCRATCH_BYTES uaesk_gcm_scratch_bytes()
static void *stream_tag_slot(uaes_gcm_stream *s) { return (char *)s->scratch + STREAM_SCRATCH_BYTES; }
static int *stream_status_slot(uaes_gcm_stream *s) { return (int *)((char *)stream_tag_slot(s) + 16); }
/* (a word that is zero between calls, for the one-launch pieces: cleared at begin, put back by their finisher) */
static unsigned *stream_done_word(uaes_gcm_stream *s) { return (unsigned *)((char *)stream_tag_slot(s) + 32); }

int uaes_gcm_stream_begin(uaes_gcm_stream **out, int keybits, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, int decrypt)
{
    context *c;
    lane *L;
    uaes_gcm_stream *s;
    const void *d_aad;
    int rc;
    if (!out || !nonce) return fail(UAES_E_ARG, "NULL pointer");
    *out = NULL;
    if ((s = (uaes_gcm_stream *)calloc(1, sizeof *s)) == NULL) return fail(UAES_E_HIP, "out of host memory");
    if ((rc = expand_key(&s->ks, key, keybits)) != 0 || (rc = enter(&c, &L)) != 0) { memset(s, 0, sizeof *s); free(s); return rc; }
    memcpy(s->nonce, nonce, 12);
    s->decrypt = decrypt != 0;
    s->aad_len = aDataLen;
    pthread_mutex_lock(&c->mu);
    if (c->nspool > 0) s->scratch = c->spool[--c->nspool];
    pthread_mutex_unlock(&c->mu);
    if (hipGetDevice(&s->device) != hipSuccess ||
        (!s->scratch && hipMalloc(&s->scratch, STREAM_SCRATCH_BYTES + 64) != hipSuccess)) {
        memset(s, 0, sizeof *s);
        free(s);
        return fail(UAES_E_HIP, "stream scratch allocation failed");
    }
    /* every call on a stream object ends with the calling thread's lane drained, so the pieces may come
     * from different threads (one at a time): the next piece is ordered behind this one by the host  */
    do {
        if (hipMemsetAsync(stream_tag_slot(s), 0, 64, (hipStream_t)L->stream) != hipSuccess) { rc = fail(UAES_E_HIP, "hipMemsetAsync failed"); break; }
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        int k = uaesk_gcm_stream_absorb(L->stream, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, 0, d_aad, aDataLen,
                                        0, 0, s->scratch, &s->plan_state);
        if (k) { rc = fail(UAES_E_HIP, "gcm stream launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = lane_sync(L);
    } while (0);
    if (rc) { (void)lane_abandon(L, rc); (void)hipFree(s->scratch); memset(s, 0, sizeof *s); free(s); return rc; }
    *out = s;
    return 0;
}

/* A stream's scratch lives on the device it was begun on; update / finish may be called
 * from a thread that is bound to another device (a multi-GPU worker): bind the stream's
 * device for the duration of the call and restore the caller's afterwards.            */
static int stream_enter(const uaes_gcm_stream *s, int *prev)
{
    HIPCHK(hipGetDevice(prev));
    if (*prev != s->device) HIPCHK(hipSetDevice(s->device));
    return 0;
}

static int stream_leave(const uaes_gcm_stream *s, int prev, int rc)
{
    if (prev != s->device && hipSetDevice(prev) != hipSuccess && rc == 0)
        rc = fail(UAES_E_HIP, "could not restore the caller's HIP device %d", prev);
    return rc;
}

static int gcm_stream_update_on_device(uaes_gcm_stream *s, const void *in, size_t len, void *outp)
{
    context *c;
    lane *L;
    io_plan io;
    uaesk_ctr ctr;
    uint8_t j0[16];
    int rc;
    if (!s || (len && (!in || !outp))) return fail(UAES_E_ARG, "NULL pointer");
    if (s->closed) return fail(UAES_E_ARG, "the stream already took its last (ragged) piece");
    if (len == 0) return 0;
    if ((rc = enter(&c, &L)) != 0) return rc;
    memcpy(j0, s->nonce, 12);
    j0[12] = j0[13] = j0[14] = 0; j0[15] = 1;
    make_ctr(&ctr, j0, 1 + s->done / 16);            /* keystream block i uses J0 + 1 + i (N4) */
    do {
        int k;
        if ((rc = plan_io(L, in, len, outp, len, &io)) != 0) break;
        /* a long piece: CTR and GHASH in one pass over it (uaesk_gcm_stream_piece; 1 = not taken) */
        k = uaesk_gcm_stream_piece(L->stream, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, s->decrypt, io.din, len, s->done, io.dout,
                                   s->scratch, &s->plan_state, stream_done_word(s));
        if (k == 0) { rc = finish_io(&io, len); break; }
        if (k != 1) { rc = fail(UAES_E_HIP, "gcm stream launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if (s->decrypt) {                             /* hash the ciphertext before it may be overwritten */
            k = uaesk_gcm_stream_absorb(L->stream, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, 1, io.din, len, 0, 0, s->scratch, &s->plan_state);
            if (!k) k = uaesk_ctr_xcrypt(L->stream, &c->tb, s->ks.nr, &s->ks.ek, &ctr, io.din, io.dout, len, NULL);
        } else {
            k = uaesk_ctr_xcrypt(L->stream, &c->tb, s->ks.nr, &s->ks.ek, &ctr, io.din, io.dout, len, NULL);
            if (!k) k = uaesk_gcm_stream_absorb(L->stream, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, 1, io.dout, len, 0, 0, s->scratch, &s->plan_state);
        }
        if (k) { rc = fail(UAES_E_HIP, "gcm stream launch: %s", hipGetErrorString((hipError_t)k)); break; }
        rc = finish_io(&io, len);
    } while (0);
    if (rc) (void)lane_abandon(L, rc);
    if (rc == 0) {
        s->done += len;
        if (len % 16) s->closed = 1;
    }
    return rc;
}

int uaes_gcm_stream_update(uaes_gcm_stream *s, const void *in, size_t len, void *outp)
{
    int prev, rc;
    if (!s) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = stream_enter(s, &prev)) != 0) return rc;
    return stream_leave(s, prev, gcm_stream_update_on_device(s, in, len, outp));
}

int uaes_gcm_stream_finish(uaes_gcm_stream *s, uint8_t tag[16])
{
    context *c;
    lane *L;
    int rc, status = -1, prev, device;
    if (!s || !tag) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = stream_enter(s, &prev)) != 0) return rc;
    device = s->device;
    if ((rc = enter(&c, &L)) != 0) { uaes_gcm_stream_abort(s); goto restore; }
    do {
        hipError_t e = hipSuccess;
        hipStream_t st = (hipStream_t)L->stream;
        int k = uaesk_gcm_stream_absorb(st, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, 2, NULL, 0,
                                        s->aad_len, s->done, s->scratch, &s->plan_state);
        if (!k && s->decrypt) e = hipMemcpyAsync(stream_tag_slot(s), tag, 16, hipMemcpyHostToDevice, st);
        if (!k && e == hipSuccess)
            k = uaesk_gcm_stream_tag(st, s->scratch, s->decrypt, stream_tag_slot(s), stream_status_slot(s));
        if (k || e != hipSuccess) { rc = fail(UAES_E_HIP, "gcm stream finish launch failed"); break; }
        if (s->decrypt) rc = lane_fetch(L, &status, stream_status_slot(s), sizeof status);
        else rc = lane_fetch(L, tag, stream_tag_slot(s), 16);
        if (rc) break;
        if (s->decrypt && status != 0) rc = UAES_E_AUTHENTICATION;
        /* everything this stream enqueued is done (lane_fetch drained the lane): wipe the scratch (H and its tables are
         * key material) and keep it for the next stream instead of hipDeviceSynchronize + hipFree */
        if (hipMemsetAsync(s->scratch, 0, STREAM_SCRATCH_BYTES + 64, st) == hipSuccess && lane_sync(L) == 0) {
            pthread_mutex_lock(&c->mu);
            if (c->nspool < (int)(sizeof c->spool / sizeof c->spool[0])) { c->spool[c->nspool++] = s->scratch; s->scratch = NULL; }
            pthread_mutex_unlock(&c->mu);
        }
    } while (0);
    if (rc < 0) (void)lane_abandon(L, rc);
    uaes_gcm_stream_abort(s);
restore:
    if (prev != device && hipSetDevice(prev) != hipSuccess && rc == 0)
        rc = fail(UAES_E_HIP, "could not restore the caller's HIP device %d", prev);
    return rc;
}

void uaes_gcm_stream_abort(uaes_gcm_stream *s)
{
    int prev = -1;
    if (!s) return;
    if (s->scratch) {
        /* hipFree works from any current device, but must not run while kernels that use the
         * buffer are in flight: every begin / update / finish drains the lane it ran on before it
         * returns, so nothing is; the device-wide wait only covers a call that failed half-way  */
        if (hipGetDevice(&prev) == hipSuccess && prev != s->device && hipSetDevice(s->device) != hipSuccess) prev = -1;
        (void)hipDeviceSynchronize();
        if (hipFree(s->scratch) != hipSuccess)
            (void)fail(UAES_E_HIP, "uaes_gcm_stream_abort: hipFree of the stream scratch failed");
        if (prev >= 0 && prev != s->device) (void)hipSetDevice(prev);
    }
    memset(s, 0, sizeof *s);                          /* key schedule */
    free(s);
}

/* ------------------------------------------------------------------------ */
/* one process, several GPUs (extension 3)                       */
/* ------------------------------------------------------------------------ */
/* The text is cut into 16-byte (CTR) or data-unit (XTS) aligned slices, one per
 * device; one host thread per device binds it (hipSetDevice is per thread) and
 * runs the ordinary single-device call on its slice with the counter / sector
 * offset advanced -- the per-device contexts make that safe.  With host buffers
 * every device moves its slice over its own PCIe link, which is what scales.  */
typedef struct {
    int         device, keybits, mode, encrypt, rc;       /* mode 0 CTR, 1 XTS sectors, 2 nothing (an empty slice),
                                                           * 3 ECB, 4 a GCM shard, 5 what a GCM-decrypt shard does once the
                                                           * tag has been judged (encrypt = the verdict: 1 good, 0 forged) */
    const uint8_t *key;
    uint8_t     ctr0[16];
    uint64_t    offset;                                   /* block offset / first sector / byte offset of a GCM shard */
    size_t      sector_bytes, nsectors;
    const void *in;
    void       *out;
    size_t      len;
    /* GCM shards */
    int         gcm_mode, padding;                        /* uaesk_gcm_shard's mode; ECB: the reference's AES_PADDING */
    const uint8_t *nonce;
    const void *aad;
    uint64_t    aad_len, total_len;
    uint8_t     share[16];
    void       *hold;                                     /* a decrypting shard's private device copy, kept until the verdict */
    char        err[256];
} mgpu_job;

static int gcm_shard_sync(int keybits, const uint8_t *key, const uint8_t *nonce, int mode,
                          const void *aData, uint64_t aDataLen, const void *in, size_t len, uint64_t off,
                          uint64_t total, void *out, uint8_t share[16]);

/* One device's part of uaes_mgpu_gcm_decrypt BEFORE the tag is known.  Nothing may reach the caller's buffer yet (N7,
 * micro_aes.c:1200-1208).  Device-reachable, aligned buffers: the shard's ciphertext is hashed where it lies (with
 * uaes_set_gcm_one_pass_decrypt: decrypted into place in the same pass and zeroed again if the tag turns out wrong).
 * Host (or misaligned) buffers: the slice goes into a device buffer of this call's own, is decrypted there in one
 * pass with the hash, and waits for the verdict -- the text crosses the link once each way.                       */
static int gcm_decrypt_shard_first(mgpu_job *j)
{
    const int direct = (j->len == 0) ||
                       (is_device_ptr(j->in) && is_device_ptr(j->out) && ((((uintptr_t)j->in) | ((uintptr_t)j->out)) & 15u) == 0);
    if (direct) {
        j->gcm_mode = (j->len && gcm_decrypt_mode() == 2) ? 2 : 1;
        return gcm_shard_sync(j->keybits, j->key, j->nonce, j->gcm_mode, j->aad, j->aad_len, j->in, j->len, j->offset,
                              j->total_len, j->out, j->share);
    }
    j->gcm_mode = 2;
    if (hipMalloc(&j->hold, j->len + 64) != hipSuccess) { j->hold = NULL; return fail(UAES_E_HIP, "no device memory for a %zu-byte shard", j->len); }
    if (hipMemcpy(j->hold, j->in, j->len, hipMemcpyDefault) != hipSuccess) return fail(UAES_E_HIP, "copying a shard in failed");
    return gcm_shard_sync(j->keybits, j->key, j->nonce, 2, j->aad, j->aad_len, j->hold, j->len, j->offset,
                          j->total_len, j->hold, j->share);
}

/* ... and once the host has XORed the shares and compared the tag */
static int gcm_decrypt_shard_second(mgpu_job *j)
{
    const int good = j->encrypt;
    int rc = 0;
    if (j->hold) {
        if (good && hipMemcpy(j->out, j->hold, j->len, hipMemcpyDefault) != hipSuccess) rc = fail(UAES_E_HIP, "copying a shard out failed");
        (void)hipMemset(j->hold, 0, j->len);              /* plaintext */
        if (hipFree(j->hold) != hipSuccess && rc == 0) rc = fail(UAES_E_HIP, "hipFree of a shard buffer failed");
        j->hold = NULL;
        return rc;
    }
    if (j->len == 0) return 0;
    if (j->gcm_mode == 2) {                               /* written already: keep it, or take it back */
        if (!good && hipMemset(j->out, 0, j->len) != hipSuccess) rc = fail(UAES_E_HIP, "wiping an unauthenticated shard failed");
        return rc;
    }
    if (!good) return 0;
    return uaes_ctr_xcrypt_at(j->keybits, j->key, j->ctr0, 1 + j->offset / 16, j->in, j->len, j->out);
}

static void *mgpu_worker(void *arg)
{
    mgpu_job *j = (mgpu_job *)arg;
    hipError_t e = hipSetDevice(j->device);
    if (e != hipSuccess) {
        j->rc = UAES_E_HIP;
        snprintf(j->err, sizeof j->err, "hipSetDevice(%d): %s", j->device, hipGetErrorString(e));
        return NULL;
    }
    switch (j->mode) {
    case 0: j->rc = uaes_ctr_xcrypt_at(j->keybits, j->key, j->ctr0, j->offset, j->in, j->len, j->out); break;
    case 1: j->rc = uaes_xts_sectors(j->keybits, j->key, j->offset, j->sector_bytes, j->nsectors, j->in, j->out, j->encrypt); break;
    case 2: return NULL;                                  /* an empty slice */
    case 3: j->rc = j->encrypt ? uaes_ecb_encrypt_padded(j->keybits, j->key, j->padding, j->in, j->len, j->out)
                               : uaes_ecb_decrypt(j->keybits, j->key, j->in, j->len, j->out); break;
    case 4: j->rc = j->encrypt ? gcm_shard_sync(j->keybits, j->key, j->nonce, 0, j->aad, j->aad_len, j->in, j->len, j->offset,
                                                j->total_len, j->out, j->share)
                               : gcm_decrypt_shard_first(j); break;
    case 5: j->rc = gcm_decrypt_shard_second(j); break;
    default: j->rc = UAES_E_ARG; snprintf(j->err, sizeof j->err, "unknown job"); return NULL;
    }
    if (j->rc < 0) snprintf(j->err, sizeof j->err, "device %d: %s", j->device, uaes_last_error());
    return NULL;
}

/* One PERSISTENT worker thread per device ordinal, started the first time a multi-GPU call names the device
 * (threads created per call also created and destroyed their per-thread lane -- a stream, pinned
 * windows, staging -- per call, milliseconds of hipHostMalloc / hipHostFree for a medium-sized text).  A call hands
 * every slice to the worker of its device and waits for all of them; slices of one device run one after the other on
 * that device's worker, slices of different devices side by side.  Calls from several host threads queue up
 * per worker.  The workers live until the process ends (they hold nothing but their lane).                  */
typedef struct mgpu_item {
    mgpu_job *job;
    int *left;                                   /* jobs of the same call still running (under done_mu) */
    pthread_mutex_t *done_mu;
    pthread_cond_t *done_cv;
    struct mgpu_item *next;
} mgpu_item;

static struct {
    pthread_t th;
    int started;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    mgpu_item *head, *tail;
} g_mgpu[MAX_DEVICES];
static pthread_mutex_t g_mgpu_start_mu = PTHREAD_MUTEX_INITIALIZER;

static void *mgpu_pool_thread(void *arg)
{
    const int d = (int)(intptr_t)arg;
    tls_is_mgpu_worker = 1;                          /* a slice is never split again (auto_devices) */
    for (;;) {
        mgpu_item *it;
        pthread_mutex_lock(&g_mgpu[d].mu);
        while (!g_mgpu[d].head) pthread_cond_wait(&g_mgpu[d].cv, &g_mgpu[d].mu);
        it = g_mgpu[d].head;
        g_mgpu[d].head = it->next;
        if (!g_mgpu[d].head) g_mgpu[d].tail = NULL;
        pthread_mutex_unlock(&g_mgpu[d].mu);
        (void)mgpu_worker(it->job);
        pthread_mutex_lock(it->done_mu);
        if (--*it->left == 0) pthread_cond_signal(it->done_cv);
        pthread_mutex_unlock(it->done_mu);
    }
    return NULL;
}

static int mgpu_pool_ensure(int d)
{
    int ok = 1;
    pthread_mutex_lock(&g_mgpu_start_mu);
    if (!g_mgpu[d].started) {
        pthread_attr_t at;
        pthread_mutex_init(&g_mgpu[d].mu, NULL);
        pthread_cond_init(&g_mgpu[d].cv, NULL);
        pthread_attr_init(&at);
        pthread_attr_setdetachstate(&at, PTHREAD_CREATE_DETACHED);
        ok = pthread_create(&g_mgpu[d].th, &at, mgpu_pool_thread, (void *)(intptr_t)d) == 0;
        pthread_attr_destroy(&at);
        g_mgpu[d].started = ok;
    }
    pthread_mutex_unlock(&g_mgpu_start_mu);
    return ok;
}

static int mgpu_run(mgpu_job *jobs, int n)
{
    mgpu_item items[MAX_DEVICES];
    pthread_mutex_t done_mu = PTHREAD_MUTEX_INITIALIZER;
    pthread_cond_t done_cv = PTHREAD_COND_INITIALIZER;
    int i, left = 0, rc = 0;
    /* uaes_set_producer_stream() is thread-local to the CALLER; the slices run on the persistent workers, whose own
     * producer stream is NULL (they wait for their device's default stream only).  Device-resident input that the
     * caller produced on a non-blocking stream is therefore waited for HERE, once, before any worker may read it
     * (ADVICE r05). */
    if (tls_producer_stream && hipStreamSynchronize((hipStream_t)tls_producer_stream) != hipSuccess)
        return fail(UAES_E_HIP, "waiting for the caller's producer stream failed: %s", hipGetErrorString(hipGetLastError()));
    for (i = 0; i < n; ++i)
        if (!mgpu_pool_ensure(jobs[i].device)) return fail(UAES_E_HIP, "pthread_create failed");
    pthread_mutex_lock(&done_mu);
    left = n;
    pthread_mutex_unlock(&done_mu);
    for (i = 0; i < n; ++i) {
        const int d = jobs[i].device;
        items[i].job = &jobs[i]; items[i].left = &left; items[i].done_mu = &done_mu; items[i].done_cv = &done_cv;
        items[i].next = NULL;
        pthread_mutex_lock(&g_mgpu[d].mu);
        if (g_mgpu[d].tail) g_mgpu[d].tail->next = &items[i]; else g_mgpu[d].head = &items[i];
        g_mgpu[d].tail = &items[i];
        pthread_cond_signal(&g_mgpu[d].cv);
        pthread_mutex_unlock(&g_mgpu[d].mu);
    }
    pthread_mutex_lock(&done_mu);
    while (left) pthread_cond_wait(&done_cv, &done_mu);
    pthread_mutex_unlock(&done_mu);
    pthread_mutex_destroy(&done_mu);
    pthread_cond_destroy(&done_cv);
    for (i = 0; i < n && rc == 0; ++i)
        if (jobs[i].rc) rc = jobs[i].rc < 0 ? fail(jobs[i].rc, "%s", jobs[i].err) : jobs[i].rc;
    return rc;
}

static int mgpu_devices(int ndev, const int *devices, int *out)
{
    int i, avail = 0;
    if (ndev < 1 || ndev > MAX_DEVICES) return fail(UAES_E_ARG, "ndev must be 1..%d (got %d)", MAX_DEVICES, ndev);
    if (hipGetDeviceCount(&avail) != hipSuccess || avail <= 0)
        return fail(UAES_E_HIP, "no usable HIP device; this library has no CPU path");
    for (i = 0; i < ndev; ++i) {
        out[i] = devices ? devices[i] : i;
        if (out[i] < 0 || out[i] >= avail) return fail(UAES_E_ARG, "device %d is not one of the %d visible", out[i], avail);
        if (out[i] >= MAX_DEVICES) return fail(UAES_E_ARG, "device %d: this library drives ordinals below %d", out[i], MAX_DEVICES);
    }
    return 0;
}

int uaes_mgpu_ctr_xcrypt_at(int ndev, const int *devices, int keybits, const uint8_t *key,
                            const uint8_t ctr0[16], uint64_t block_offset,
                            const void *in, size_t len, void *out)
{
    mgpu_job jobs[MAX_DEVICES];
    int dev[MAX_DEVICES], i, rc, n = 0;
    const size_t blocks = (len + 15) / 16;
    if (!key || !ctr0 || (len && (!in || !out))) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = mgpu_devices(ndev, devices, dev)) != 0) return rc;
    memset(jobs, 0, sizeof jobs);
    for (i = 0; i < ndev; ++i) {
        const size_t b0 = blocks * (size_t)i / (size_t)ndev, b1 = blocks * (size_t)(i + 1) / (size_t)ndev;
        const size_t lo = b0 * 16, hi = b1 * 16 < len ? b1 * 16 : len;
        if (hi <= lo) continue;
        jobs[n].device = dev[i]; jobs[n].keybits = keybits; jobs[n].key = key; jobs[n].mode = 0;
        memcpy(jobs[n].ctr0, ctr0, 16);
        jobs[n].offset = block_offset + b0;
        jobs[n].in = (const char *)in + lo; jobs[n].out = (char *)out + lo; jobs[n].len = hi - lo;
        ++n;
    }
    return n ? mgpu_run(jobs, n) : 0;
}

int uaes_mgpu_xts_sectors(int ndev, const int *devices, int keybits, const uint8_t *keys,
                          uint64_t first_sector, size_t sector_bytes, size_t nsectors,
                          const void *in, void *out, int encrypt)
{
    mgpu_job jobs[MAX_DEVICES];
    int dev[MAX_DEVICES], i, rc, n = 0;
    if (!keys || (nsectors && (!in || !out))) return fail(UAES_E_ARG, "NULL pointer");
    if (sector_bytes < 16) return UAES_E_DATALENGTH;
    if ((rc = mgpu_devices(ndev, devices, dev)) != 0) return rc;
    memset(jobs, 0, sizeof jobs);
    for (i = 0; i < ndev; ++i) {
        const size_t s0 = nsectors * (size_t)i / (size_t)ndev, s1 = nsectors * (size_t)(i + 1) / (size_t)ndev;
        if (s1 <= s0) continue;
        jobs[n].device = dev[i]; jobs[n].keybits = keybits; jobs[n].key = keys; jobs[n].mode = 1;
        jobs[n].encrypt = encrypt; jobs[n].offset = first_sector + s0;
        jobs[n].sector_bytes = sector_bytes; jobs[n].nsectors = s1 - s0;
        jobs[n].in = (const char *)in + s0 * sector_bytes; jobs[n].out = (char *)out + s0 * sector_bytes;
        ++n;
    }
    return n ? mgpu_run(jobs, n) : 0;
}

/* ECB (AES_ECB_encrypt / AES_ECB_decrypt, micro_aes.c:636-680): any partition of the blocks will do.  The whole
 * blocks are dealt out evenly; the last slice also takes the ragged tail and the padding (N1, padBlock :610-621), so
 * what is written -- and a decryption's 0x1D for a length that is no multiple of 16 (:679) -- is the one-device result. */
static int mgpu_ecb(int ndev, const int *devices, int keybits, const uint8_t *key, int encrypt, int padding,
                    const void *in, size_t len, void *out)
{
    mgpu_job jobs[MAX_DEVICES];
    int dev[MAX_DEVICES], i, rc, n = 0;
    const size_t nfull = len / 16;
    if (!key || (len && (!in || !out)) || (encrypt && padding && !out)) return fail(UAES_E_ARG, "NULL pointer");
    if (padding < 0 || padding > 2) return fail(UAES_E_ARG, "padding %d (0 zeros, 1 PKCS#7, 2 ISO 7816-4)", padding);
    if ((rc = mgpu_devices(ndev, devices, dev)) != 0) return rc;
    memset(jobs, 0, sizeof jobs);
    for (i = 0; i < ndev; ++i) {
        const int last = i == ndev - 1;
        const size_t lo = nfull * (size_t)i / (size_t)ndev * 16, hi = last ? len : nfull * (size_t)(i + 1) / (size_t)ndev * 16;
        if (hi <= lo && !(last && encrypt && padding)) continue;      /* (PKCS#7 / ISO padding always appends a block) */
        jobs[n].device = dev[i]; jobs[n].keybits = keybits; jobs[n].key = key; jobs[n].mode = 3;
        jobs[n].encrypt = encrypt; jobs[n].padding = last ? padding : 0;
        jobs[n].in = (const char *)in + lo; jobs[n].out = (char *)out + lo; jobs[n].len = hi - lo;
        ++n;
    }
    return n ? mgpu_run(jobs, n) : 0;
}

int uaes_mgpu_ecb_encrypt(int ndev, const int *devices, int keybits, const uint8_t *key, int padding,
                          const void *pntxt, size_t ptextLen, void *crtxt)
{
    return mgpu_ecb(ndev, devices, keybits, key, 1, padding, pntxt, ptextLen, crtxt);
}

int uaes_mgpu_ecb_decrypt(int ndev, const int *devices, int keybits, const uint8_t *key,
                          const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return mgpu_ecb(ndev, devices, keybits, key, 0, 0, crtxt, crtxtLen, pntxt);
}

/* ------------------------------------------------------------------------ */
/* GCM over several GPUs (CTR shards + one 16-byte exchange)     */
/* ------------------------------------------------------------------------ */
/* One shard of a GCM message on the calling thread's current device, synchronously: the CTR pass (mode 0 / 2) fused
 * with the shard's weighted share of Enc(J0) ^ GHASH (uaesk_gcm_shard); mode 1 hashes only.  in / out host or device. */
static int gcm_shard_sync(int keybits, const uint8_t *key, const uint8_t *nonce, int mode,
                          const void *aData, uint64_t aDataLen, const void *in, size_t len, uint64_t off,
                          uint64_t total, void *out, uint8_t share[16])
{
    context *c;
    lane *L;
    keysched ks;
    io_plan io;
    const void *d_aad = NULL;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        int k;
        if ((rc = gcm_scratch(L, SCRATCH_OTHER)) != 0) break;
        if (off == 0 && (rc = stage_aad(L, aData, (size_t)aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, in, len, mode == 1 ? NULL : out, mode == 1 ? 0 : len, &io)) != 0) break;
        k = uaesk_gcm_shard(L->stream, &c->tb, ks.nr, &ks.ek, mode, nonce, d_aad, aDataLen, io.din, len, off, total,
                            mode == 1 ? NULL : io.dout, L->scratch, L->d_status + 4);
        if (k) { rc = fail(UAES_E_HIP, "gcm shard launch: %s", hipGetErrorString((hipError_t)k)); break; }
        if ((rc = lane_fetch(L, share, L->d_status + 4, 16)) != 0) break;
        if (mode != 1) { io.drained = 1; rc = finish_io(&io, len); }
    } while (0);
    memset(&ks, 0, sizeof ks);
    DONE(L, rc);
}

/* the 16 bytes behind a text that may be host or device memory */
static int tag_store(void *dst, const uint8_t tag[16])
{
    if (!is_device_ptr(dst)) { memcpy(dst, tag, 16); return 0; }
    if (hipMemcpy(dst, tag, 16, hipMemcpyDefault) != hipSuccess) return fail(UAES_E_HIP, "writing the tag failed");
    return 0;
}

static int tag_load(uint8_t tag[16], const void *src)
{
    if (!is_device_ptr(src)) { memcpy(tag, src, 16); return 0; }
    if (hipMemcpy(tag, src, 16, hipMemcpyDefault) != hipSuccess) return fail(UAES_E_HIP, "reading the tag failed");
    return 0;
}

/* the shards of a len-byte text: 16-byte aligned slices, the first one at offset 0 (it carries the AAD and Enc(J0)),
 * the last one ending at len (it carries the length block); a text too short for every device leaves some out, and
 * an EMPTY text still is one shard (its tag is Enc(J0) ^ GHASH(AAD, lengths))                                     */
static int gcm_shard_jobs(mgpu_job *jobs, int ndev, const int *dev, int keybits, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, const void *in, size_t len, void *out, int encrypt)
{
    const size_t blocks = (len + 15) / 16;
    int i, n = 0;
    for (i = 0; i < ndev; ++i) {
        const size_t b0 = blocks * (size_t)i / (size_t)ndev, b1 = blocks * (size_t)(i + 1) / (size_t)ndev;
        const size_t lo = b0 * 16, hi = b1 * 16 < len ? b1 * 16 : len;
        if (hi <= lo && !(len == 0 && i == 0)) continue;
        memset(&jobs[n], 0, sizeof jobs[n]);
        jobs[n].device = dev[i]; jobs[n].keybits = keybits; jobs[n].key = key; jobs[n].mode = 4; jobs[n].encrypt = encrypt;
        jobs[n].nonce = nonce; jobs[n].aad = aData; jobs[n].aad_len = aDataLen; jobs[n].total_len = len;
        j0_of_nonce12(nonce, jobs[n].ctr0);
        jobs[n].offset = lo;
        jobs[n].in = len ? (const char *)in + lo : NULL; jobs[n].out = len ? (char *)out + lo : NULL; jobs[n].len = hi - lo;
        ++n;
    }
    return n;
}

int uaes_mgpu_gcm_encrypt(int ndev, const int *devices, int keybits, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, const void *pntxt, size_t ptextLen, void *crtxt)
{
    mgpu_job jobs[MAX_DEVICES];
    uint8_t tag[16] = { 0 };
    int dev[MAX_DEVICES], i, k, rc, n;
    if (!key || !nonce || !crtxt || (ptextLen && !pntxt) || (aDataLen && !aData)) return fail(UAES_E_ARG, "NULL pointer");
    if (keybits != 128 && keybits != 192 && keybits != 256) return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if ((rc = mgpu_devices(ndev, devices, dev)) != 0) return rc;
    n = gcm_shard_jobs(jobs, ndev, dev, keybits, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt, 1);
    if ((rc = mgpu_run(jobs, n)) != 0) return rc;
    for (i = 0; i < n; ++i)
        for (k = 0; k < 16; ++k) tag[k] ^= jobs[i].share[k];
    return tag_store((char *)crtxt + ptextLen, tag);
}

/* N7 across devices (micro_aes.c:1200-1208): every device first produces its share of the tag over the INPUT; the host
 * XORs them and compares; only then does any device write the caller's buffer.  A forgery returns 0x1A with every
 * shard untouched (or, for device buffers under uaes_set_gcm_one_pass_decrypt, zeroed -- as the one-device call does). */
int uaes_mgpu_gcm_decrypt(int ndev, const int *devices, int keybits, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, const void *crtxt, size_t crtxtLen, void *pntxt)
{
    mgpu_job jobs[MAX_DEVICES];
    uint8_t tag[16] = { 0 }, given[16];
    int dev[MAX_DEVICES], i, k, rc, rc2, n, good;
    if (!key || !nonce || !crtxt || (crtxtLen && !pntxt) || (aDataLen && !aData)) return fail(UAES_E_ARG, "NULL pointer");
    if (keybits != 128 && keybits != 192 && keybits != 256) return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if ((rc = mgpu_devices(ndev, devices, dev)) != 0) return rc;
    if ((rc = tag_load(given, (const char *)crtxt + crtxtLen)) != 0) return rc;
    n = gcm_shard_jobs(jobs, ndev, dev, keybits, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt, 0);
    rc = mgpu_run(jobs, n);
    for (i = 0; i < n; ++i)
        for (k = 0; k < 16; ++k) tag[k] ^= jobs[i].share[k];
    good = rc == 0 && !tags_differ(tag, given, 16);
    for (i = 0; i < n; ++i) { jobs[i].mode = 5; jobs[i].encrypt = good; jobs[i].rc = 0; }
    if (rc != 0) {                                         /* a device failed: the others still give their buffers back */
        char msg[256];
        snprintf(msg, sizeof msg, "%s", uaes_last_error());
        (void)mgpu_run(jobs, n);
        return rc < 0 ? fail(rc, "%s", msg) : rc;
    }
    rc2 = mgpu_run(jobs, n);
    if (rc2 != 0) return rc2;
    return good ? 0 : UAES_E_AUTHENTICATION;
}

/* ------------------------------------------------------------------------ */
/* CTR over several GPUs with the ciphertext gathered on one of them over xGMI */
/* (BASELINE configs[4]; north_star: "RCCL over xGMI only for the final         */
/* ciphertext gather", host code in C).  RCCL is a SOFT dependency: librccl.so  */
/* is opened with dlopen the first time more than one device takes part, and a  */
/* box without it gets UAES_E_HIP with the loader's message, not a link error.  */
/* ------------------------------------------------------------------------ */
typedef struct { char internal[128]; } rccl_unique_id;
typedef void *rccl_comm;
typedef struct {
    void *handle;
    int (*CommInitAll)(rccl_comm *comms, int ndev, const int *devlist);
    int (*CommDestroy)(rccl_comm comm);
    int (*CommAbort)(rccl_comm comm);                     /* optional: NULL when the library has none */
    int (*CommCount)(const rccl_comm comm, int *count);   /* optional */
    int (*GroupStart)(void);
    int (*GroupEnd)(void);
    int (*Send)(const void *buf, size_t count, int dtype, int peer, rccl_comm comm, hipStream_t st);
    int (*Recv)(void *buf, size_t count, int dtype, int peer, rccl_comm comm, hipStream_t st);
    const char *(*GetErrorString)(int rc);
    int tried;
    char err[256];
} rccl_api;
#define RCCL_UINT8 1                                      /* ncclUint8 (nccl.h: ncclInt8 = 0, ncclUint8 = 1) */

static rccl_api g_rccl;
static pthread_mutex_t g_rccl_mu = PTHREAD_MUTEX_INITIALIZER;

/* the communicators of ONE device list are kept for the life of the process: ncclCommInitAll costs seconds */
static struct {
    int ndev, devs[MAX_DEVICES], ready;
    rccl_comm comm[MAX_DEVICES];
    hipStream_t stream[MAX_DEVICES];
} g_gather;

static int rccl_load(void)
{
    static const char *names[] = { NULL, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so" };
    size_t i;
    if (g_rccl.handle) return 0;
    if (g_rccl.tried) return fail(UAES_E_HIP, "RCCL is not available: %s", g_rccl.err);
    g_rccl.tried = 1;
    names[0] = getenv("UAES_RCCL_LIB");
    for (i = 0; i < sizeof names / sizeof names[0] && !g_rccl.handle; ++i) {
        if (!names[i] || !*names[i]) continue;
        g_rccl.handle = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
        if (!g_rccl.handle) snprintf(g_rccl.err, sizeof g_rccl.err, "%s", dlerror());
        if (i == 0 && !g_rccl.handle) break;              /* an explicit UAES_RCCL_LIB that does not load is an error, not a hint */
    }
    if (!g_rccl.handle) return fail(UAES_E_HIP, "RCCL is not available: %s", g_rccl.err);
#define RCCL_SYM(field, name) \
    do { *(void **)&g_rccl.field = dlsym(g_rccl.handle, name); \
         if (!g_rccl.field) { snprintf(g_rccl.err, sizeof g_rccl.err, "%s not found in librccl", name); \
                              dlclose(g_rccl.handle); g_rccl.handle = NULL; return fail(UAES_E_HIP, "RCCL is not available: %s", g_rccl.err); } } while (0)
    RCCL_SYM(CommInitAll, "ncclCommInitAll"); RCCL_SYM(CommDestroy, "ncclCommDestroy");
    RCCL_SYM(GroupStart, "ncclGroupStart");   RCCL_SYM(GroupEnd, "ncclGroupEnd");
    RCCL_SYM(Send, "ncclSend");               RCCL_SYM(Recv, "ncclRecv");
    RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
    *(void **)&g_rccl.CommAbort = dlsym(g_rccl.handle, "ncclCommAbort");
    *(void **)&g_rccl.CommCount = dlsym(g_rccl.handle, "ncclCommCount");
    return 0;
}

/* Two switches for the test suite and the one-GPU bench line, read on every call (a gather moves megabytes: a getenv
 * is nothing beside it).  UAES_GATHER_FORCE_RCCL=1: slices that live on the root's own device and were encrypted into
 * shard buffers of their own also travel by ncclSend / ncclRecv -- rank r to rank r inside the group, which RCCL
 * allows -- instead of hipMemcpy, so that a box with ONE GPU runs the loader, the hand-declared prototypes,
 * RCCL_UINT8, the communicator cache and the drain below.  UAES_GATHER_FAIL_SEND=k (k >= 1): the k-th send of the
 * call is issued with a peer rank that does not exist, so RCCL itself refuses it (ncclInvalidArgument) in the middle
 * of an open group with k-1 transfers already enqueued. */
static int gather_force_rccl(void)
{
    const char *e = getenv("UAES_GATHER_FORCE_RCCL");
    return e && *e && *e != '0';
}

static int gather_fail_send(void)
{
    const char *e = getenv("UAES_GATHER_FAIL_SEND");
    return e && *e ? atoi(e) : 0;
}

static struct { unsigned long sends, recvs, groups, inits, failures; } g_gather_stats;

/* ---- the table of arrangements as data (csrc/uaes_plan.h; include/uaes_hip.h) ---- */
int uaes_debug_plan_at(int mode, int dir, size_t a, size_t b, unsigned flags, const uint8_t counter16[16], int out[4])
{
    uaes_plan p;
    int e;
    if (!out) return fail(UAES_E_ARG, "NULL pointer");
    memset(&p, 0, sizeof p);
    if ((e = uaesk_plan_at(mode, dir, a, b, flags, counter16, &p)) != 0) return fail(UAES_E_ARG, "no plan for mode %d, direction %d", mode, dir);
    out[0] = p.arrangement; out[1] = p.launches; out[2] = (int)p.grid; out[3] = (int)p.steps;
    return 0;
}
int uaes_debug_plan(int mode, int dir, size_t a, size_t b, unsigned flags, int out[4])
{
    return uaes_debug_plan_at(mode, dir, a, b, flags, NULL, out);
}
const char *uaes_debug_arrangement_name(int id) { return uaesk_arrangement_name(id); }
const char *uaes_debug_plan_poly1305(size_t len, size_t nmsg, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    (void)uaesk_plan_poly1305(len, nmsg, &p);
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; }
    return uaesk_poly1305_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_eax_siv(int siv, int dir, size_t len, size_t nmsg, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (uaesk_plan_eax_siv(siv, dir, len, nmsg, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)UAES_EAX_SIV_SMALL_MAX; }
    return uaesk_eax_siv_arrangement_name(p.arrangement);
}
void uaes_debug_plan_disable(unsigned mask) { uaesk_plan_disable(mask); }

/* ---- test hooks of the one-launch GCM arrangements (include/uaes_hip.h) ---- */
void uaes_debug_gcm_look(unsigned long long ticks_100mhz) { uaesk_debug_gcm_look(ticks_100mhz); }

int uaes_debug_gcm_chunk_folds(unsigned *out)
{
    context *c;
    int rc;
    if (!out) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = get_context(&c)) != 0) return rc;
    KCHK(hipDeviceSynchronize());
    KCHK(uaesk_debug_gcm_chunk_folds(out));
    return 0;
}

/* how often each RCCL entry point has run in this process (tests: "the gather really went through RCCL") */
void uaes_debug_gather_stats(unsigned long out[5])
{
    pthread_mutex_lock(&g_rccl_mu);
    out[0] = g_gather_stats.sends; out[1] = g_gather_stats.recvs; out[2] = g_gather_stats.groups;
    out[3] = g_gather_stats.inits; out[4] = g_gather_stats.failures;
    pthread_mutex_unlock(&g_rccl_mu);
}

/* forget the communicators and streams of the cached device list (mutex held).  After a failed transfer the
 * communicators are in a state RCCL does not define: they are aborted (ncclCommAbort, where the library has it)
 * rather than destroyed, and the next gather builds fresh ones. */
static void gather_drop_locked(int after_failure)
{
    int i, prev = -1;
    if (!g_gather.ready) return;
    (void)hipGetDevice(&prev);
    for (i = 0; i < g_gather.ndev; ++i) {
        if (after_failure && g_rccl.CommAbort) (void)g_rccl.CommAbort(g_gather.comm[i]);
        else (void)g_rccl.CommDestroy(g_gather.comm[i]);
        if (hipSetDevice(g_gather.devs[i]) == hipSuccess) (void)hipStreamDestroy(g_gather.stream[i]);
    }
    g_gather.ready = 0;
    if (prev >= 0) (void)hipSetDevice(prev);
}

static void gather_teardown(void)
{
    pthread_mutex_lock(&g_rccl_mu);
    gather_drop_locked(0);
    pthread_mutex_unlock(&g_rccl_mu);
}

static int rccl_fail(const char *what, int rc)
{
    return fail(UAES_E_HIP, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
}

/* communicators + one stream per device for this device list (mutex held) */
static int gather_setup(int ndev, const int *dev)
{
    int i, rc, prev = -1;
    if (g_gather.ready && g_gather.ndev == ndev && memcmp(g_gather.devs, dev, (size_t)ndev * sizeof *dev) == 0) return 0;
    (void)hipGetDevice(&prev);
    gather_drop_locked(0);                                 /* another device list: start over */
    for (i = 0; i < ndev; ++i)
        if (hipSetDevice(dev[i]) != hipSuccess || hipStreamCreateWithFlags(&g_gather.stream[i], hipStreamNonBlocking) != hipSuccess) {
            while (--i >= 0) if (hipSetDevice(dev[i]) == hipSuccess) (void)hipStreamDestroy(g_gather.stream[i]);
            if (prev >= 0) (void)hipSetDevice(prev);
            return fail(UAES_E_HIP, "stream creation for the gather failed");
        }
    rc = g_rccl.CommInitAll(g_gather.comm, ndev, dev);
    if (prev >= 0) (void)hipSetDevice(prev);
    if (rc != 0) {
        for (i = 0; i < ndev; ++i) if (hipSetDevice(dev[i]) == hipSuccess) (void)hipStreamDestroy(g_gather.stream[i]);
        if (prev >= 0) (void)hipSetDevice(prev);
        return rccl_fail("ncclCommInitAll", rc);
    }
    ++g_gather_stats.inits;
    if (g_rccl.CommCount) {                                /* the hand-declared prototypes against the library: ask it */
        int cnt = -1;
        if (g_rccl.CommCount(g_gather.comm[0], &cnt) != 0 || cnt != ndev) {
            memcpy(g_gather.devs, dev, (size_t)ndev * sizeof *dev);
            g_gather.ndev = ndev; g_gather.ready = 1;
            gather_drop_locked(1);
            return fail(UAES_E_HIP, "ncclCommCount says %d ranks, %d were set up", cnt, ndev);
        }
    }
    memcpy(g_gather.devs, dev, (size_t)ndev * sizeof *dev);
    g_gather.ndev = ndev;
    g_gather.ready = 1;
    return 0;
}

int uaes_mgpu_ctr_encrypt_gather(int ndev, const int *devices, int keybits, const uint8_t *key,
                                 const uint8_t ctr0[16], uint64_t block_offset,
                                 const void *const *d_in, size_t len, void *const *d_out,
                                 int root, void *d_full_on_root)
{
    mgpu_job jobs[MAX_DEVICES];
    size_t lo[MAX_DEVICES], hi[MAX_DEVICES];
    int dev[MAX_DEVICES], i, rc, prev = -1;
    const size_t blocks = (len + 15) / 16;
    if (!key || !ctr0 || (len && (!d_in || !d_full_on_root))) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = mgpu_devices(ndev, devices, dev)) != 0) return rc;
    if (root < 0 || root >= ndev) return fail(UAES_E_ARG, "root %d is not one of the %d devices", root, ndev);
    if (!len) return 0;
    memset(jobs, 0, sizeof jobs);
    for (i = 0; i < ndev; ++i) {
        const size_t b0 = blocks * (size_t)i / (size_t)ndev, b1 = blocks * (size_t)(i + 1) / (size_t)ndev;
        lo[i] = b0 * 16; hi[i] = b1 * 16 < len ? b1 * 16 : len;
        if (hi[i] < lo[i]) hi[i] = lo[i];
        if (hi[i] > lo[i] && !d_in[i]) return fail(UAES_E_ARG, "no input shard for device %d", dev[i]);
        if (hi[i] > lo[i] && dev[i] != dev[root] && (!d_out || !d_out[i])) return fail(UAES_E_ARG, "no output shard for device %d", dev[i]);
        jobs[i].device = dev[i]; jobs[i].keybits = keybits; jobs[i].key = key; jobs[i].mode = hi[i] > lo[i] ? 0 : 2;
        memcpy(jobs[i].ctr0, ctr0, 16);
        jobs[i].offset = block_offset + b0;
        jobs[i].in = hi[i] > lo[i] ? d_in[i] : NULL;
        /* a slice on the root's device is encrypted straight into its place in the gathered text unless the caller
         * also wants it in a shard buffer of its own */
        {
            void *own = d_out ? d_out[i] : NULL;
            jobs[i].out = (dev[i] == dev[root] && !own) ? (void *)((char *)d_full_on_root + lo[i]) : own;
        }
        jobs[i].len = hi[i] - lo[i];
    }
    if ((rc = mgpu_run(jobs, ndev)) != 0) return rc;
    (void)hipGetDevice(&prev);
    {
        /* slices that live on the root's own device (its own, and those of a device list that names the device more
         * than once) are device-to-device copies -- unless UAES_GATHER_FORCE_RCCL sends them through RCCL as well; the
         * others travel by RCCL, one send / receive pair each */
        int uniq[MAX_DEVICES], rank_of[MAX_DEVICES], by_rccl[MAX_DEVICES], nu = 0, remote = 0, u;
        const int force = gather_force_rccl(), fail_at = gather_fail_send();
        for (i = 0; i < ndev; ++i) {
            const int in_place = jobs[i].out == (void *)((char *)d_full_on_root + lo[i]);
            for (u = 0; u < nu && uniq[u] != dev[i]; ++u) { }
            if (u == nu) uniq[nu++] = dev[i];
            rank_of[i] = u;
            by_rccl[i] = hi[i] > lo[i] && !in_place && (dev[i] != dev[root] || force);
            if (by_rccl[i]) ++remote;
        }
        if (hipSetDevice(dev[root]) != hipSuccess) rc = fail(UAES_E_HIP, "hipSetDevice(%d) failed", dev[root]);
        for (i = 0; i < ndev && rc == 0; ++i) {
            if (dev[i] != dev[root] || hi[i] == lo[i] || by_rccl[i] || jobs[i].out == (void *)((char *)d_full_on_root + lo[i])) continue;
            if (hipMemcpy((char *)d_full_on_root + lo[i], jobs[i].out, hi[i] - lo[i], hipMemcpyDeviceToDevice) != hipSuccess)
                rc = fail(UAES_E_HIP, "copying a local slice into place failed: %s", hipGetErrorString(hipGetLastError()));
        }
        if (rc == 0 && remote) {
            int g, started = 0, nsend = 0;
            pthread_mutex_lock(&g_rccl_mu);
            rc = rccl_load();
            if (rc == 0) rc = gather_setup(nu, uniq);
            if (rc == 0 && (g = g_rccl.GroupStart()) != 0) rc = rccl_fail("ncclGroupStart", g);
            if (rc == 0) {
                started = 1;
                ++g_gather_stats.groups;
                for (i = 0; i < ndev && rc == 0; ++i) {
                    if (!by_rccl[i]) continue;
                    /* the injected failure: a destination rank the communicator does not have */
                    const int to = (++nsend == fail_at) ? nu + 7 : rank_of[root];
                    if ((g = g_rccl.Send(jobs[i].out, hi[i] - lo[i], RCCL_UINT8, to, g_gather.comm[rank_of[i]],
                                         g_gather.stream[rank_of[i]])) != 0)
                        rc = rccl_fail("ncclSend", g);
                    else if (++g_gather_stats.sends,
                             (g = g_rccl.Recv((char *)d_full_on_root + lo[i], hi[i] - lo[i], RCCL_UINT8, rank_of[i],
                                              g_gather.comm[rank_of[root]], g_gather.stream[rank_of[root]])) != 0)
                        rc = rccl_fail("ncclRecv", g);
                    else ++g_gather_stats.recvs;
                }
            }
            if (started && (g = g_rccl.GroupEnd()) != 0 && rc == 0) rc = rccl_fail("ncclGroupEnd", g);
            /* drained whatever happened: after a failed send / receive the ones already enqueued may still be writing
             * d_full_on_root and reading the shard buffers, and the caller is about to get those back */
            for (u = 0; u < nu && g_gather.ready; ++u)
                if ((hipSetDevice(uniq[u]) != hipSuccess || hipStreamSynchronize(g_gather.stream[u]) != hipSuccess) && rc == 0)
                    rc = fail(UAES_E_HIP, "the gather did not complete on device %d: %s", uniq[u], hipGetErrorString(hipGetLastError()));
            if (rc != 0) {                                 /* whatever state the group left them in: not reused */
                ++g_gather_stats.failures;
                gather_drop_locked(1);
            }
            pthread_mutex_unlock(&g_rccl_mu);
        }
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return rc;
}
