/*
 * uaes_engine.c -- core of the host layer of the MI355X AES engine (plain C).
 *
 * What every mode needs and no mode owns: error reporting and the policy switches, table generation, the key
 * schedule (KeyExpansion, micro_aes.c:144-178 -- host side, <= 240 bytes of output), the per-device contexts,
 * per-thread lanes and completion tickets, the environment settings, staging of host buffers, the slice pipeline,
 * the housekeeping API and the debug hooks.  The modes' entry points live in uaes_engine_modes.c, uaes_engine_gcm.c
 * and uaes_engine_mgpu.c; what they may touch of this file is declared in uaes_engine.h.
 *
 * By default ALL block-cipher and GHASH work happens in the HIP kernels behind uaes_device.h, and a missing or
 * failed HIP device is reported, never papered over.  The one exception is opt-in: the host data path of
 * uaes_host.c, which a deployer switches on (uaes_set_host_policy / UAES_HOST_*) and which the synchronous entry
 * points then ask for through host_take() before they go to the GPU.
 */
#include "uaes_engine.h"

#define UAES_VERSION "uaes-hip 0.1 gfx950"

/* ------------------------------------------------------------------------ */
/* errors                                                                     */
/* ------------------------------------------------------------------------ */
static __thread char tls_err[256];

static int g_device_suspect;                       /* set by every UAES_E_HIP: the host fallback looks at the device again */
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tls_err, sizeof tls_err, fmt, ap);
    va_end(ap);
    if (code == UAES_E_HIP) __atomic_store_n(&g_device_suspect, 1, __ATOMIC_RELEASE);
    return code;
}

/* what a kernel launcher (uaes_device.h) answered: 0, or the runtime's error under the name of what was launched */
int launched(const char *what, int k)
{
    return k ? fail(UAES_E_HIP, "%s launch: %s", what, hipGetErrorString((hipError_t)k)) : 0;
}

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

int wipe_on_auth_failure(void) { return __atomic_load_n(&g_wipe_on_auth_failure, __ATOMIC_ACQUIRE); }
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

int gcm_decrypt_mode(void) { return __atomic_load_n(&g_gcm_one_pass, __ATOMIC_ACQUIRE) ? 2 : 1; }

/* tag comparison whose run time does not depend on where the tags differ */
int tags_differ(const uint8_t *a, const uint8_t *b, size_t n)
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

/* schedules expanded and not yet wiped, process-wide (uaes_debug_live_key_schedules) */
static int g_live_schedules;

void burn(void *p, size_t n)
{
    volatile unsigned char *v = (volatile unsigned char *)p;
    while (n--) *v++ = 0;
}

/* burn()'s effect at memset's speed (the byte-wise volatile loop was 0.1 us of every call, profiles/key_wipe_latency.md):
 * the empty asm may read the memory for all the compiler knows, so the stores stay */
void keysched_wipe(keysched *sched)
{
    if (sched->nr) __atomic_fetch_sub(&g_live_schedules, 1, __ATOMIC_RELAXED);
    memset(sched, 0, sizeof *sched);
    __asm__ __volatile__("" : : "r"(sched) : "memory");
}

int expand_key(keysched *ks, const uint8_t *key, int keybits)
{
    int nk, total, i;
    uint8_t rcon = 1;
    ks->nr = 0;
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
    __atomic_fetch_add(&g_live_schedules, 1, __ATOMIC_RELAXED);
    return 0;
}

/* diagnostic export: lets the CPU test-suite check the schedule without a GPU */
int uaes_expand_key(int keybits, const uint8_t *key, uint32_t enc_words[60], uint32_t dec_words[60])
{
    KEYSCHED(ks);
    int rc = expand_key(&ks, key, keybits);
    if (rc) return rc;
    if (enc_words) memcpy(enc_words, ks.ek.w, sizeof ks.ek.w);
    if (dec_words) memcpy(dec_words, ks.dk.w, sizeof ks.dk.w);
    return ks.nr;
}

/* ------------------------------------------------------------------------ */
/* per-device context                                                         */
/* ------------------------------------------------------------------------ */

static context g_ctx[MAX_DEVICES];
static pthread_mutex_t g_init_mu = PTHREAD_MUTEX_INITIALIZER;

int get_context(context **out)
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
            __atomic_store_n(&c->ready, 1, __ATOMIC_RELEASE);
        }
        pthread_mutex_unlock(&g_init_mu);
    }
    *out = c;
    return 0;
}

int grow_on(void *stream, void **buf, size_t *cap, size_t need)
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

unsigned *scratch_done_word(void *buf, size_t cap)
{
    return (unsigned *)((char *)buf + cap - SCRATCH_TAIL);
}

/* The word the calling thread armed last (arm_done_word) and the stream its call ran on.  The workgroups of a
 * one-launch call restore the zero themselves; a call that did NOT run to its end -- a launch the runtime refused, a
 * sequence abandoned half-way -- may not have, and a count left behind would make the next call on that word fold too
 * early.  Every failure path therefore puts the zero back, in stream order behind whatever did get queued
 * (lane_abandon, and any non-zero launch rc). */
static __thread unsigned *tls_armed_word;
void arm_done_word(unsigned *w)
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
void disarm_done_word_dev(void *stream, int launch_rc)
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
int scratch_pin(context *c, void *stream, size_t need, void **buf, int *slot_out)
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

void scratch_unpin(context *c, int k)
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

/* anything else that writes the lane's scratch (XTS chunk tweaks, OCB rows, GHASH under a foreign H ...) */
void lane_scratch_clobbered(lane *L)
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
int enter(context **c, lane **L)
{
    int rc = get_context(c);
    return rc ? rc : get_lane(*c, L);
}

/* The lane's scratch, for `owner`.  SCRATCH_GCM_KEYED: a GCM call under the lane's cached key -- the only user that
 * leaves the key's tables valid (lane_gcm_keyed decides whether they are there).  Anybody else (XTS chunk tweaks, OCB
 * rows, GHASH under a foreign H, GCM-SIV, a GCM shard ...) is about to overwrite them: asking for the buffer IS the
 * invalidation, no writer has to remember a second call. */
int lane_scratch(lane *L, size_t need, int owner)
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

int gcm_key_cache_enabled(void)
{
    env_ready();
    return g_env.gcm_key_cache;
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
void ticket_arm(lane *L, size_t text_bytes)
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

/* wait until everything queued on the lane's stream is done; n > 0: also bring n bytes (<= 64, a multiple of 4)
 * from device memory `dev` to `host`                                                                        */
int lane_wait_fetch(lane *L, void *host, const void *dev, size_t n)
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

/* Where a synchronous call's kernels put their status word (0 / 0x1A): a word of the lane's pinned page when there
 * is one -- the host then reads it as soon as the stream has drained, no copy command, and a one-launch decryption can
 * carry the completion ticket itself -- else the lane's device slot.                                            */
int *lane_status(lane *L)
{
    if (ticket_enabled() && pinned_ready(L)) return (int *)((char *)L->pinx + TICKET_OFF + 16);
    return L->d_status;
}

/* wait for the lane, then the status word its kernels wrote through `where` (= lane_status(L)) */
int lane_read_status(lane *L, int *where, int *status)
{
    int rc;
    if (where == L->d_status) return lane_fetch(L, status, L->d_status, sizeof *status);
    if ((rc = lane_sync(L)) != 0) return rc;
    *status = *(volatile int *)where;
    return 0;
}

int is_device_ptr(const void *p)
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

int wait_for_callers_device_work(void)
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

void *producer_stream(void) { return tls_producer_stream; }

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
void mgpu_worker_enter(void) { tls_is_mgpu_worker = 1; }

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
 *   chains     ONE serial chain given host pointers -- CBC / CFB encryption, OFB, CMAC, CCM, key wrap, FF1, FF3-1 -- runs on the host whatever
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

/* leaving through the host path: a non-zero code gets its text in uaes_last_error() like the device path's */
int host_result(int rc)
{
    if (rc == UAES_E_AUTHENTICATION) return fail(rc, "authentication failed (host path)");
    if (rc == UAES_E_DECRYPTION) return fail(rc, "ciphertext length is no multiple of the block size (host path)");
    if (rc == UAES_E_DATALENGTH) return fail(rc, "data too short (host path)");
    if (rc != 0) return fail(rc, "host path failed (%d)", rc);
    return 0;
}

/* does this call run on the host path?  chain != 0: one serial chain; gcm != 0: GCM's own, lower crossover applies */
int host_take_mode(const void *in, const void *out, size_t len, int chain, int gcm)
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

/* > 1: split this call over devs[0..n); 0: run it on the current device as always */
int auto_devices(const void *in, const void *out, size_t len, int *devs)
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

/* Short host texts travel through pinned bounce buffers with asynchronous copies on the
 * lane's stream, so a call synchronises once instead of three times (pageable hipMemcpy
 * in, kernel, pageable hipMemcpy out): ~45 -> ~28 us for a 4 KiB call.  Shorter ones still
 * (zero_copy_max()) are not copied at all: the pinned buffers are mapped into the GPU's address
 * space, so the kernel reads the text from pin[0] and writes the result to pin[1] across the
 * link itself -- one submission per call instead of three (copy, kernel, copy).          */

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

int plan_io(lane *L, const void *in, size_t in_len, void *out, size_t out_cap, io_plan *io)
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

int finish_io(io_plan *io, size_t out_len)
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
int lane_abandon(lane *L, int rc)
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
#define PIPE_MAXW     16

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

int pipe_workers(void)
{
    env_ready();
    return g_env.pipe_workers;
}

size_t pipe_slice_bytes(void)
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
        if (k > 0 && launched("slice", k)) PFAIL(j, "%s", uaes_last_error());
        if (k < 0) PFAIL(j, "slice at offset %zu: %s", off, uaes_last_error());   /* this thread's message */
        e = hipMemcpyAsync(j->out + off, d, olen, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) PFAIL(j, "slice copy out: %s", hipGetErrorString(e));
    }
}

/* returns 1 if the call qualifies (both buffers plain host memory, long enough), and then *rc is its result */
int run_pipelined(context *c, const void *in, void *out, size_t total, size_t unit, size_t out_extra,
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
int finish_io_unauthenticated(io_plan *io, size_t out_len)
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
int dev_ptrs_ok(const void *in, const void *out, size_t len)
{
    if (len && (!in || !out)) return fail(UAES_E_ARG, "NULL device pointer");
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 15u)
        return fail(UAES_E_ARG, "device pointers of the *_dev API must be 16-byte aligned");
    return 0;
}

/* the synchronous entry points run between enter() and DONE(): the latter drains the lane when the
 * call did not end in finish_io / lane_fetch (an error in the middle)                              */
int lane_leave(lane *L, int rc)
{
    if (rc < 0) rc = lane_abandon(L, rc);
    tls_armed_word = NULL;                           /* the word may belong to a key context the caller frees next */
    return rc;
}

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
    KEYSCHED(ks);
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
        if ((rc = launched("selftest", k)) != 0) break;
        if ((rc = lane_fetch(L, &result, d, 4)) != 0) break;
        rc = (int)result;
    } while (0);
    DONE(L, rc);
}

/* ------------------------------------------------------------------------ */
/* staging helpers of the entry points (modes, GCM, multi-GPU)                 */
/* ------------------------------------------------------------------------ */
int gcm_scratch(lane *L, int owner)       /* synchronous API: the thread's own scratch */
{
    return lane_scratch(L, uaesk_gcm_scratch_bytes(), owner);
}

/* the *_dev entry points do not hold the context lock while the GPU works (they only
 * enqueue), but growing the shared scratch buffer must not race with another thread */
int gcm_scratch_locked(context *c, void *stream, void **scr, int *slot)
{
    int rc;
    pthread_mutex_lock(&c->mu);
    rc = scratch_pin(c, stream, uaesk_gcm_scratch_bytes(), scr, slot);
    pthread_mutex_unlock(&c->mu);
    return rc;
}

/* AAD may be host memory: stage it (it is read byte-wise, no alignment need) */
int stage_aad(lane *L, const void *aad, size_t aad_len, const void **d_aad)
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

/* J0 of GCM's default 12-byte nonce: nonce || 00000001 (any other length: gcm_j0, uaes_engine_gcm.c) */
void j0_of_nonce12(const uint8_t *nonce, uint8_t j0[16])
{
    memcpy(j0, nonce, 12);
    j0[12] = j0[13] = j0[14] = 0;
    j0[15] = 1;
}

/* the counter block of the CTR kernels: ctr0 + block_offset in its low 56 bits */
void make_ctr(uaesk_ctr *c, const uint8_t ctr0[16], uint64_t block_offset)
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

/* side arrays (nonce, AAD, tags) in host memory travel through the lane's scratch, SIDE(n) bytes each */
int side_in(lane *L, size_t *off, const void *src, size_t n, const void **d)
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
int iv_read(uint8_t out[16], const uint8_t *iv)
{
    if (is_device_ptr(iv)) { HIPCHK(hipMemcpy(out, iv, 16, hipMemcpyDeviceToHost)); }
    else memcpy(out, iv, 16);
    return 0;
}
int iv_write(uint8_t *iv, const uint8_t v[16])
{
    if (is_device_ptr(iv)) { HIPCHK(hipMemcpy(iv, v, 16, hipMemcpyHostToDevice)); }
    else memcpy(iv, v, 16);
    return 0;
}

int stage_text(lane *L, int k, const void *user, size_t n, int prefill, void **d)
{
    if (!n) { *d = NULL; return 0; }
    if (is_device_ptr(user)) { *d = (void *)user; return wait_for_callers_device_work(); }
    if (grow_on(L->stream, &L->stage[k], &L->stage_cap[k], n + 64)) return UAES_E_HIP;
    *d = L->stage[k];
    if (prefill) HIPCHK(hipMemcpyAsync(*d, user, n, hipMemcpyHostToDevice, (hipStream_t)L->stream));
    return 0;
}

/* ---- a row batch's arrays (uaes_engine_modes.c: aead_rows_staged for every AEAD record batch -- EAX, SIV, CCM,
 * GCM-SIV, multi-key GCM and OCB -- cipher_rows for the batches of the plain cipher modes, and the key-wrap, FF1 and
 * FF3-1 batches) ----
 * The caller lists its side arrays (row_array, uaes_engine.h) and its two texts (row_text) and calls row_stage,
 * row_texts, its launcher and row_finish, in this order.  A device array goes to the kernel as it is; host arrays
 * share the lane's scratch, SIDE(bytes) each.  The offsets and the size asked of lane_scratch come from the one list,
 * so no array can lie past the end.  row_stage waits for the caller's device work, once for the whole list, if any
 * listed array, read or written, is device memory (row_texts waits again for each text that is: stage_text);
 * status != 0: the kernel reports through L->d_status[0], cleared here. */
int row_stage(lane *L, row_array *a, int n, int status)
{
    size_t need = 0, off = 0;
    int i, rc, dev = 0;
    for (i = 0; i < n; ++i) {
        a[i].d = NULL;
        if (!a[i].bytes) continue;
        if (is_device_ptr(a[i].user)) { a[i].d = (void *)a[i].user; dev = 1; }
        else need += SIDE(a[i].bytes);
    }
    if (need && (rc = lane_scratch(L, need, SCRATCH_OTHER)) != 0) return rc;
    for (i = 0; i < n; ++i) {
        if (!a[i].bytes || a[i].d) continue;
        a[i].d = (char *)L->scratch + off;
        off += SIDE(a[i].bytes);
        if (!a[i].out) HIPCHK(hipMemcpyAsync(a[i].d, a[i].user, a[i].bytes, hipMemcpyHostToDevice, (hipStream_t)L->stream));
    }
    if (dev && (rc = wait_for_callers_device_work()) != 0) return rc;
    if (status) HIPCHK(hipMemsetAsync(L->d_status, 0, sizeof(int), (hipStream_t)L->stream));
    return 0;
}

int row_texts(lane *L, row_text *t)
{
    const int rc = stage_text(L, 0, t->in, t->in_bytes, 1, &t->d_in);
    return rc ? rc : stage_text(L, 1, t->out, t->out_bytes, t->prefill, &t->d_out);
}

/* everything the kernel wrote into staging goes back to the caller, with the status word if the call has one
 * (else *bad = 0): one synchronise, one round trip */
int row_finish(lane *L, const row_text *t, const row_array *a, int n, int status, int *bad)
{
    hipStream_t st = (hipStream_t)L->stream;
    int i;
    *bad = 0;
    if (t->out_bytes && t->d_out != t->out) HIPCHK(hipMemcpyAsync(t->out, t->d_out, t->out_bytes, hipMemcpyDeviceToHost, st));
    for (i = 0; i < n; ++i)
        if (a[i].out && a[i].bytes && a[i].d != a[i].user)
            HIPCHK(hipMemcpyAsync((void *)a[i].user, a[i].d, a[i].bytes, hipMemcpyDeviceToHost, st));
    if (status) HIPCHK(hipMemcpyAsync(bad, L->d_status, sizeof *bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

/* the 16 bytes behind a text that may be host or device memory */
int tag_store(void *dst, const uint8_t tag[16])
{
    if (!is_device_ptr(dst)) { memcpy(dst, tag, 16); return 0; }
    if (hipMemcpy(dst, tag, 16, hipMemcpyDefault) != hipSuccess) return fail(UAES_E_HIP, "writing the tag failed");
    return 0;
}

int tag_load(uint8_t tag[16], const void *src)
{
    if (!is_device_ptr(src)) { memcpy(tag, src, 16); return 0; }
    if (hipMemcpy(tag, src, 16, hipMemcpyDefault) != hipSuccess) return fail(UAES_E_HIP, "reading the tag failed");
    return 0;
}

/* ------------------------------------------------------------------------ */
/* debug hooks (include/uaes_hip.h)                                           */
/* ------------------------------------------------------------------------ */
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
const char *uaes_debug_plan_eaxp(int dir, size_t len, size_t nmsg, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (uaesk_plan_eaxp(dir, len, nmsg, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)UAES_EAX_SIV_SMALL_MAX; }
    return uaesk_eax_siv_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_siv_v(int dir, size_t len, size_t nad, size_t nmsg, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (uaesk_plan_siv_v(dir, len, nad, nmsg, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; }
    return uaesk_eax_siv_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_chain(int what, int dir, size_t a, size_t b, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (what == UAES_WHAT_CCM_BATCH ? uaesk_plan_ccm_batch(dir, a, b, &p)
        : what == UAES_WHAT_CMAC || what == UAES_WHAT_CCM ? uaesk_plan_mac(what, dir, a, &p) : uaesk_plan_chain(what, dir, a, b, &p))
        return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; }
    return uaesk_chain_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_ff1(int dir, unsigned radix, size_t len, size_t nrec, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (uaesk_plan_ff1(dir, radix, len, nrec, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; }
    return uaesk_ff1_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_ff3(int dir, unsigned radix, size_t len, size_t nrec, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (uaesk_plan_ff3(dir, radix, len, nrec, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; }
    return uaesk_ff3_arrangement_name(p.arrangement);
}
/* the hook of a planner that takes (dir, len, nmsg) -- the row batches and the two key wraps: the plan under its
 * arrangement's name; NULL for arguments the planner refuses */
static const char *debug_plan_rows(int (*plan)(int, size_t, size_t, uaes_plan *), const char *(*name)(int), int dir, size_t len,
                                   size_t nmsg, int out[3])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (plan(dir, len, nmsg, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; }
    return name(p.arrangement);
}
const char *uaes_debug_plan_kw(int dir, size_t len, size_t nkeys, int out[3])
{
    return debug_plan_rows(uaesk_plan_kw, uaesk_kw_arrangement_name, dir, len, nkeys, out);
}
const char *uaes_debug_plan_kwp(int dir, size_t len, size_t nkeys, int out[3])
{
    return debug_plan_rows(uaesk_plan_kwp, uaesk_kwp_arrangement_name, dir, len, nkeys, out);
}
const char *uaes_debug_plan_gcmsiv_batch(int dir, size_t len, size_t nmsg, int out[3])
{
    return debug_plan_rows(uaesk_plan_gcmsiv_batch, uaesk_gcmsiv_batch_arrangement_name, dir, len, nmsg, out);
}
const char *uaes_debug_plan_gcm_multikey_batch(int dir, size_t len, size_t nmsg, int out[3])
{
    return debug_plan_rows(uaesk_plan_gcm_multikey_batch, uaesk_gcm_multikey_arrangement_name, dir, len, nmsg, out);
}
const char *uaes_debug_plan_xaes256gcm_batch(int dir, size_t len, size_t nmsg, int out[3])
{
    return debug_plan_rows(uaesk_plan_xaes_gcm_batch, uaesk_xaes_gcm_arrangement_name, dir, len, nmsg, out);
}
const char *uaes_debug_plan_ocb_batch(int dir, size_t len, size_t nmsg, int out[3])
{
    return debug_plan_rows(uaesk_plan_ocb_batch, uaesk_ocb_batch_arrangement_name, dir, len, nmsg, out);
}
const char *uaes_debug_plan_cipher_batch(int mode, size_t len, size_t nmsg, int out[3])
{
    return debug_plan_rows(uaesk_plan_cipher_batch, uaesk_cipher_batch_arrangement_name, mode, len, nmsg, out);
}
/* out = { launches, workgroups, threads per workgroup, units per workgroup } */
const char *uaes_debug_plan_xts_batch(size_t len, size_t nmsg, int out[4])
{
    uaes_plan p;
    memset(&p, 0, sizeof p);
    if (uaesk_plan_xts_batch(len, nmsg, &p)) return NULL;
    if (out) { out[0] = p.launches; out[1] = (int)p.grid; out[2] = (int)p.steps; out[3] = (int)(p.steps / 16u); }
    return uaesk_xts_batch_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_ocb(int dir, size_t len, size_t aad_len, int aad_aligned, int out[5])
{
    uaes_plan p;
    int shape[5];
    memset(&p, 0, sizeof p);
    if (uaesk_plan(UAES_PLAN_OCB, dir, len, aad_len, 0, &p)) return NULL;
    if (p.arrangement == UAES_ARR_OCB_RUNS) {
        if (uaesk_plan_ocb_shape(dir, len, aad_len, aad_aligned, shape)) return NULL;
        if (out) memcpy(out, shape, sizeof shape);
    }
    return uaesk_arrangement_name(p.arrangement);
}
const char *uaes_debug_plan_xts(size_t sector_bytes, size_t nsectors, int explicit_tweak, uint64_t out[8])
{
    uaes_plan p;
    uint64_t shape[8];
    memset(&p, 0, sizeof p);
    if (uaesk_plan_xts_shape(sector_bytes, nsectors, explicit_tweak, shape)) return NULL;
    if (uaesk_plan(UAES_PLAN_XTS, 0, sector_bytes, nsectors, explicit_tweak ? 2u : 0u, &p)) return NULL;
    if (out) memcpy(out, shape, sizeof shape);
    return uaesk_arrangement_name(p.arrangement);
}
int uaes_debug_plan_gcm_piece(int decrypt, size_t len, uint64_t done_bytes, int out[4])
{
    uaes_plan p;
    if (!out) return fail(UAES_E_ARG, "NULL pointer");
    memset(&p, 0, sizeof p);
    if (uaesk_plan_gcm_piece(decrypt, len, done_bytes, &p)) return fail(UAES_E_ARG, "no piece plan behind %llu bytes", (unsigned long long)done_bytes);
    out[0] = p.arrangement; out[1] = p.launches; out[2] = (int)p.grid; out[3] = (int)p.steps;
    return 0;
}
void uaes_debug_plan_disable(unsigned mask) { uaesk_plan_disable(mask); }

int uaes_debug_live_key_schedules(void) { return __atomic_load_n(&g_live_schedules, __ATOMIC_RELAXED); }

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
