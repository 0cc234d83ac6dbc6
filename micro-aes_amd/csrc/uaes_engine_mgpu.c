/*
 * uaes_engine_mgpu.c -- one process, several GPUs: the jobs and the persistent worker pool behind uaes_mgpu_*, the
 * RCCL loader and the xGMI gather.  The workers call the ordinary single-device entry points for their slices.
 */
#include <dlfcn.h>

#include "uaes_engine.h"

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
    mgpu_worker_enter();                             /* a slice is never split again (auto_devices) */
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
    if (producer_stream() && hipStreamSynchronize((hipStream_t)producer_stream()) != hipSuccess)
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

void gather_teardown(void)
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
