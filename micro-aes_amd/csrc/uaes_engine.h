/*
 * uaes_engine.h -- INTERNAL to the engine's host layer (csrc/ only, never installed): what uaes_engine_modes.c,
 * uaes_engine_gcm.c and uaes_engine_mgpu.c may touch of the core in uaes_engine.c, and the few functions they call
 * of each other.  The types, the macros every entry point is written with, and prototypes of exactly the functions
 * that are called across files; everything declared here has hidden visibility, so the library exports what
 * include/uaes_hip.h names and nothing else.  File-scope state stays in the file that owns it.
 */
#ifndef UAES_ENGINE_H
#define UAES_ENGINE_H

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

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

#define MAX_DEVICES  16

#pragma GCC visibility push(hidden)

/* ---- errors ---- */
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

/* ---- key schedule ---- */
typedef struct {
    int      nr;                    /* 0: never expanded, or wiped */
    uaesk_rk ek, dk;
} keysched;

/* A schedule on the stack is declared with KEYSCHED(ks); at the top of its function (before any label), never as a
 * plain local: every way out of the scope then wipes it (keysched_wipe; the reference BURNs its RoundKey after every
 * call, micro_aes.c:360), also one taken before expand_key was reached (nr = 0 is all the declaration sets: the rest
 * is expand_key's to fill).  A keysched is handed on by pointer only.                                              */
void keysched_wipe(keysched *ks);
#define KEYSCHED(name) keysched name __attribute__((cleanup(keysched_wipe))); name.nr = 0

/* ---- per-device context and per-thread lanes ---- */
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

/* The last SCRATCH_TAIL bytes of a scratch buffer (lanes, *_dev slots) are words that are ZERO BETWEEN CALLS: the
 * workgroups of a one-launch call count themselves in on one and the last arrival puts the zero back (uaesk_ocb's
 * done_word).  Cleared when the buffer is allocated, on the stream that uses it; no kernel's scratch layout
 * reaches them (every request is made SCRATCH_TAIL bytes larger).                                            */
#define SCRATCH_TAIL 256u
enum { SCRATCH_OTHER = 0, SCRATCH_GCM_KEYED = 1 };

/* ---- staging of the caller's buffers, the slice pipeline ---- */
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

typedef int (*pipe_launch_fn)(void *arg, int worker, void *stream, const void *d_in, void *d_out, size_t off, size_t len);

#define DONE(L, rc) return lane_leave((L), (rc))

#define PIPE_MIN      ((size_t)32 << 20)          /* shorter texts: the plain path            */

/* enqueue with the pinned scratch, then drop the pin */
#define KCHK_PINNED(c, slot, call)                                                        \
    do {                                                                                  \
        int e_ = (call);                                                                  \
        scratch_unpin((c), (slot));                                                       \
        if (e_ != 0)                                                                      \
            return fail(UAES_E_HIP, "%s failed: %s", #call, hipGetErrorString((hipError_t)e_)); \
    } while (0)

#define SIDE(n) (((n) + 15) & ~(size_t)15)

/* a row batch's side arrays and texts, as its host function lists them (row_stage, uaes_engine.c) */
typedef struct {
    const void *user;               /* the caller's array, host or device memory (const for the inputs' sake:
                                     * row_stage and row_finish cast it back for an array with out = 1)       */
    size_t      bytes;              /* 0: this call has no such array, and d stays NULL                        */
    int         out;                /* 0: the kernel reads it; 1: it writes it and row_finish brings it back  */
    void       *d;                  /* row_stage's answer: where the kernel finds it                           */
} row_array;
typedef struct {
    const void *in;
    void       *out;
    size_t      in_bytes, out_bytes;
    int         prefill;            /* the output's staging starts as a copy of the caller's buffer: the kernel
                                     * leaves part of it unwritten                                             */
    void       *d_in, *d_out;       /* row_texts' answer */
} row_text;

/* ---- uaes_engine.c ---- */
int fail(int code, const char *fmt, ...);
int launched(const char *what, int k);
int wipe_on_auth_failure(void);
int gcm_decrypt_mode(void);
int tags_differ(const uint8_t *a, const uint8_t *b, size_t n);
int expand_key(keysched *ks, const uint8_t *key, int keybits);
int get_context(context **out);
int grow_on(void *stream, void **buf, size_t *cap, size_t need);
unsigned *scratch_done_word(void *buf, size_t cap);
void arm_done_word(unsigned *w);
void disarm_done_word_dev(void *stream, int launch_rc);
int scratch_pin(context *c, void *stream, size_t need, void **buf, int *slot_out);
void scratch_unpin(context *c, int k);
void lane_scratch_clobbered(lane *L);
int enter(context **c, lane **L);
int lane_scratch(lane *L, size_t need, int owner);
int gcm_key_cache_enabled(void);
void ticket_arm(lane *L, size_t text_bytes);
int lane_wait_fetch(lane *L, void *host, const void *dev, size_t n);
int *lane_status(lane *L);
int lane_read_status(lane *L, int *where, int *status);
int is_device_ptr(const void *p);
int wait_for_callers_device_work(void);
void *producer_stream(void);
void mgpu_worker_enter(void);
void burn(void *p, size_t n);
int host_result(int rc);
int host_take_mode(const void *in, const void *out, size_t len, int chain, int gcm);
int auto_devices(const void *in, const void *out, size_t len, int *devs);
int plan_io(lane *L, const void *in, size_t in_len, void *out, size_t out_cap, io_plan *io);
int finish_io(io_plan *io, size_t out_len);
int lane_abandon(lane *L, int rc);
int pipe_workers(void);
size_t pipe_slice_bytes(void);
int run_pipelined(context *c, const void *in, void *out, size_t total, size_t unit, size_t out_extra,
                  pipe_launch_fn fn, void *arg, int *rc);
int finish_io_unauthenticated(io_plan *io, size_t out_len);
int dev_ptrs_ok(const void *in, const void *out, size_t len);
int lane_leave(lane *L, int rc);
int gcm_scratch(lane *L, int owner);
int gcm_scratch_locked(context *c, void *stream, void **scr, int *slot);
int stage_aad(lane *L, const void *aad, size_t aad_len, const void **d_aad);
void j0_of_nonce12(const uint8_t *nonce, uint8_t j0[16]);
void make_ctr(uaesk_ctr *c, const uint8_t ctr0[16], uint64_t block_offset);
int side_in(lane *L, size_t *off, const void *src, size_t n, const void **d);
int iv_read(uint8_t out[16], const uint8_t *iv);
int iv_write(uint8_t *iv, const uint8_t v[16]);
int stage_text(lane *L, int k, const void *user, size_t n, int prefill, void **d);
int row_stage(lane *L, row_array *a, int n, int status);
int row_texts(lane *L, row_text *t);
int row_finish(lane *L, const row_text *t, const row_array *a, int n, int status, int *bad);
int tag_store(void *dst, const uint8_t tag[16]);
int tag_load(uint8_t tag[16], const void *src);

/* ---- uaes_engine_gcm.c ---- */
int gcm_shard_sync(int keybits, const uint8_t *key, const uint8_t *nonce, int mode,
                   const void *aData, uint64_t aDataLen, const void *in, size_t len, uint64_t off,
                   uint64_t total, void *out, uint8_t share[16]);
void xaes_k1(const keysched *mk, uint8_t k1[16]);

/* ---- uaes_engine_mgpu.c ---- */
void gather_teardown(void);

/* ---- wrappers small enough to be worth a copy in every file ---- */
static inline void ticket_armed_launch_done(lane *L)
{
    if (uaesk_ticket_disarm()) L->armed = 0;                  /* nobody took it */
}
static inline int lane_sync(lane *L)
{
    return lane_wait_fetch(L, NULL, NULL, 0);
}
/* 4 .. 16 bytes of result (status word, tag, MAC) from the lane's device slot to the host */
static inline int lane_fetch(lane *L, void *host, const void *dev, size_t n)
{
    return lane_wait_fetch(L, host, dev, n);
}

static inline int host_take(const void *in, const void *out, size_t len, int chain) { return host_take_mode(in, out, len, chain, 0); }
static inline uaesh_key host_key(const keysched *ks)
{
    uaesh_key k;
    k.ek = ks->ek.w; k.dk = ks->dk.w; k.nr = ks->nr;
    return k;
}

#pragma GCC visibility pop

#endif /* UAES_ENGINE_H */
