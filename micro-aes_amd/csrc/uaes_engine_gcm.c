/*
 * uaes_engine_gcm.c -- GCM entry points of the host layer (AES_GCM_*, micro_aes.c:1164-1212): one-shot calls and the
 * lane's cached key, key contexts and record batches, the partial / shard / GHASH building blocks, GCM-SIV,
 * streamed GCM and the synchronous shard the multi-GPU workers run.  On top of the core (uaes_engine.c, through
 * uaes_engine.h).
 */
#include "uaes_engine.h"

/* ------------------------------------------------------------------------ */
/* GCM                                                                        */
/* ------------------------------------------------------------------------ */
/* 1: the tables of `key` are in the lane's scratch (this call may run as a call on a key context, uaesk_gcm's keyed),
 * 0: they are not (the one-shot path), < 0: error.  Call with the scratch allocated (gcm_scratch).  A call on a key
 * context is 2-4 us shorter than a one-shot call and the table set costs ~20 us once, so it is built when the EIGHTH
 * call in a row comes under one key (a sequence that stops there has lost those 20 us, a longer one gains 10-15 %
 * per call); UAES_GCM_KEY_CACHE=0 switches the cache off.                                                     */
#define GK_BUILD_AT 8
#define GK_TABLES   255
static int lane_gcm_keyed(lane *L, const keysched *ks, const uint8_t *key, int keybits)
{
    const size_t kb = (size_t)keybits / 8;
    if (!gcm_key_cache_enabled() || !L->c->tb.frob) return 0;
    if (L->gk_state && L->gk_bits == keybits && memcmp(L->gk, key, kb) == 0) {
        if (L->gk_state == GK_TABLES) return 1;
        if (++L->gk_state < GK_BUILD_AT) return 0;
        const int rc = launched("key table", uaesk_gcm_key_tables(L->stream, &L->c->tb, ks->nr, &ks->ek, L->scratch));
        if (rc) return rc;
        L->gk_state = GK_TABLES;
        return 1;
    }
    memset(L->gk, 0, sizeof L->gk);
    memcpy(L->gk, key, kb);
    L->gk_bits = keybits;
    L->gk_state = 1;
    return 0;
}

/* J0 (GCMsetup, micro_aes.c:1140-1152): nonce || 00000001 for the default 12-byte nonce; for any
 * other length GHASH_H(nonce) computed on the GPU and read back (16 bytes; the counter arithmetic of
 * every kernel is a launch argument).  The lane's scratch has been sized by the caller.          */
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

/* What a GCM call runs on, whichever front door it came through: the one-shot calls (the lane's scratch, keyed once
 * lane_gcm_keyed has built the key's tables there) and the calls on a key context (its own scratch, always keyed). */
typedef struct {
    const keysched *ks;             /* by pointer only (KEYSCHED) */
    int             keyed;          /* `scratch` holds the tables of ks: uaesk_gcm's keyed */
    void           *scratch;
    unsigned       *done_word;      /* the zero-between-calls word behind `scratch` */
} gcm_how;

/* The kernels always produce the 16-byte tag behind the text; a shorter tag (the one-shot calls only) is the host
 * layer's business: the text goes through a buffer with room for sixteen bytes and ptextLen + tag_len bytes are handed
 * over (micro_aes.c:1178). */
static int gcm_encrypt_on_lane(context *c, lane *L, const gcm_how *how, const uint8_t j0[16], size_t tag_len,
                               const void *aData, size_t aDataLen, const void *pntxt, size_t ptextLen, void *crtxt)
{
    io_plan io;
    const void *d_aad;
    int rc, k;
    if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) return rc;
    if ((rc = plan_io(L, pntxt, ptextLen, crtxt, ptextLen + tag_len, &io)) != 0) return rc;
    if (tag_len < 16 && io.dout == crtxt) {
        /* the caller's own device buffer ends tag_len bytes behind the text: run into staging, copy back */
        if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], ptextLen + 64)) return UAES_E_HIP;
        io.dout = L->stage[1];
        io.copy_back = 1;
    }
    ticket_arm(L, ptextLen);
    arm_done_word(how->done_word);
    k = uaesk_gcm(L->stream, &c->tb, how->ks->nr, &how->ks->ek, 0, j0, d_aad, aDataLen, io.din, ptextLen, io.dout,
                  how->scratch, NULL, how->keyed);
    arm_done_word(NULL);
    ticket_armed_launch_done(L);
    if ((rc = launched("gcm", k)) != 0) return rc;
    return finish_io(&io, ptextLen + tag_len);
}

/* Nothing reaches the caller's buffer before the whole text has been authenticated (N7). */
static int gcm_decrypt_on_lane(context *c, lane *L, const gcm_how *how, const uint8_t j0[16], size_t tag_len,
                               const void *aData, size_t aDataLen, const void *crtxt, size_t crtxtLen, void *pntxt)
{
    io_plan io;
    const void *d_aad;
    int rc, k, status = -1;
    if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) return rc;
    /* input is CT || tag; output is crtxtLen bytes */
    if ((rc = plan_io(L, crtxt, crtxtLen + tag_len, pntxt, crtxtLen, &io)) != 0) return rc;
    if (tag_len < 16) {
        /* a truncated tag (GCM_TAG_LEN < 16, :1204) is compared here: the device computes the full tag of the
         * ciphertext (nothing is decrypted), its first tag_len bytes are checked against the ones behind the
         * text in constant time, and only then does the CTR pass write the caller's buffer (N7)          */
        uint8_t full[16], given[16];
        k = uaesk_gcm(L->stream, &c->tb, how->ks->nr, &how->ks->ek, 3, j0, d_aad, aDataLen, io.din, crtxtLen, NULL,
                      how->scratch, L->d_status + 4, how->keyed);
        if ((rc = launched("gcm", k)) != 0) return rc;
        if ((rc = lane_fetch(L, full, L->d_status + 4, 16)) != 0) return rc;
        if (is_device_ptr(io.din)) {
            if (hipMemcpy(given, (const char *)io.din + crtxtLen, tag_len, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(UAES_E_HIP, "reading the tag back failed");
        } else {
            memcpy(given, (const char *)io.din + crtxtLen, tag_len);    /* the mapped pinned window */
        }
        if (tags_differ(full, given, tag_len)) return UAES_E_AUTHENTICATION;
        k = uaesk_gcm_ctr(L->stream, &c->tb, how->ks->nr, &how->ks->ek, j0, io.din, crtxtLen, io.dout);
        if ((rc = launched("gcm", k)) != 0) return rc;
        return finish_io(&io, crtxtLen);
    }
    if (io.dout == io.din && io.copy_back) {
        /* host -> host: decrypt into the second staging buffer so that a
         * failed authentication can leave the caller's buffer untouched   */
        if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], crtxtLen + 64)) return UAES_E_HIP;
        io.dout = L->stage[1];
    }
    /* a private staging buffer may be written before the tag is known: one pass */
    const int dmode = io.copy_back || io.dout == L->pin[1] ? 2 : gcm_decrypt_mode();
    int *st_where = lane_status(L);
    if (st_where != L->d_status) { *(volatile int *)st_where = -1; ticket_arm(L, crtxtLen); }   /* host-visible status: a
                                                 * one-launch decryption may carry the completion ticket itself */
    arm_done_word(how->done_word);
    k = uaesk_gcm(L->stream, &c->tb, how->ks->nr, &how->ks->ek, dmode, j0, d_aad, aDataLen, io.din, crtxtLen, io.dout,
                  how->scratch, st_where, how->keyed);
    arm_done_word(NULL);
    ticket_armed_launch_done(L);
    if ((rc = launched("gcm", k)) != 0) return rc;
    if ((rc = lane_read_status(L, st_where, &status)) != 0) return rc;
    if (status != 0) return UAES_E_AUTHENTICATION;            /* N7: pntxt untouched */
    io.drained = 1;
    return finish_io(&io, crtxtLen);
}

/* The checks of the one-shot calls.  nonceLen / tagLen = the reference's compile-time GCM_NONCE_LEN / GCM_TAG_LEN
 * (micro_aes.h:108-109); `tagged` is the buffer that holds the tag (never NULL), `text` the other one. */
static int gcm_args_ok(const uint8_t *nonce, size_t nonceLen, size_t tagLen, const void *aData, size_t aDataLen,
                       const void *tagged, const void *text, size_t len)
{
    if (!nonce || !tagged || (len && !text)) return fail(UAES_E_ARG, "NULL pointer");
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "GCM tag length %zu (1..16)", tagLen);
    if (nonceLen == 0) return fail(UAES_E_ARG, "empty GCM nonce");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    return 0;
}

/* The lane's scratch made ready for a one-shot call under `key`: whether it holds the key's tables, and the call's J0.
 * cache == 0: a key that no later call repeats (XAES-256-GCM: it belongs to the nonce), so the lane does not remember it. */
static int gcm_lane_prepare(lane *L, keysched *ks, const uint8_t *key, int keybits, int cache, const uint8_t *nonce,
                            size_t nonceLen, int *keyed, uint8_t j0[16])
{
    int rc;
    if ((rc = gcm_scratch(L, SCRATCH_GCM_KEYED)) != 0) return rc;
    /* (before anything of this call writes the scratch under its key.  A one-shot setup builds only the tables its
     * message reaches and leaves the others undefined: with a nonce whose J0 is a GHASH of its own, which runs such
     * a setup, the call stays one-shot and the cache starts over) */
    *keyed = cache && nonceLen == 12 ? lane_gcm_keyed(L, ks, key, keybits) : 0;
    if (*keyed < 0) return *keyed;
    if (!cache || nonceLen != 12) lane_scratch_clobbered(L);
    return gcm_j0(L, ks, nonce, nonceLen, j0);
}

/* One GCM encryption under the expanded `key`, whichever front door it came through: uaes_gcm_encrypt_ex, and
 * uaes_xaes256gcm_encrypt with the key of its nonce (cache == 0, gcm_lane_prepare). */
static int gcm_encrypt_call(keysched *ks, const uint8_t *key, int keybits, int cache, const uint8_t *nonce, size_t nonceLen,
                            size_t tagLen, const void *aData, size_t aDataLen, const void *pntxt, size_t ptextLen, void *crtxt)
{
    context *c;
    lane *L;
    uint8_t j0[16];
    int rc, keyed;
    if ((rc = gcm_args_ok(nonce, nonceLen, tagLen, aData, aDataLen, crtxt, pntxt, ptextLen)) != 0) return rc;
    if (host_take_mode(pntxt, crtxt, ptextLen, 0, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(ks);
        return host_result(uaesh_gcm(&hk, 0, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)pntxt, ptextLen, (uint8_t *)crtxt));
    }
    if (nonceLen == 12 && tagLen == 16) {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(pntxt, crtxt, ptextLen, devs);
        if (nd) return uaes_mgpu_gcm_encrypt(nd, devs, keybits, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
        if (gcm_encrypt_pipelined(ks, nonce, aData, aDataLen, pntxt, ptextLen, crtxt, &rc)) return rc;
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    if ((rc = gcm_lane_prepare(L, ks, key, keybits, cache, nonce, nonceLen, &keyed, j0)) == 0) {
        const gcm_how how = { ks, keyed, L->scratch, scratch_done_word(L->scratch, L->scratch_cap) };
        rc = gcm_encrypt_on_lane(c, L, &how, j0, tagLen, aData, aDataLen, pntxt, ptextLen, crtxt);
    }
    DONE(L, rc);
}

int uaes_gcm_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    KEYSCHED(ks);
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    return gcm_encrypt_call(&ks, key, keybits, 1, nonce, nonceLen, tagLen, aData, aDataLen, pntxt, ptextLen, crtxt);
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

/* ... and one GCM decryption: uaes_gcm_decrypt_ex and uaes_xaes256gcm_decrypt */
static int gcm_decrypt_call(keysched *ks, const uint8_t *key, int keybits, int cache, const uint8_t *nonce, size_t nonceLen,
                            size_t tagLen, const void *aData, size_t aDataLen, const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    uint8_t j0[16];
    int rc, keyed;
    if ((rc = gcm_args_ok(nonce, nonceLen, tagLen, aData, aDataLen, crtxt, pntxt, crtxtLen)) != 0) return rc;
    if (host_take_mode(crtxt, pntxt, crtxtLen, 0, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(ks);
        return host_result(uaesh_gcm(&hk, 1, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)crtxt, crtxtLen, (uint8_t *)pntxt));
    }
    if (nonceLen == 12 && tagLen == 16) {
        int devs[MAX_DEVICES];
        const int nd = auto_devices(crtxt, pntxt, crtxtLen, devs);
        if (nd) return uaes_mgpu_gcm_decrypt(nd, devs, keybits, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    if ((rc = gcm_lane_prepare(L, ks, key, keybits, cache, nonce, nonceLen, &keyed, j0)) == 0) {
        const gcm_how how = { ks, keyed, L->scratch, scratch_done_word(L->scratch, L->scratch_cap) };
        rc = gcm_decrypt_on_lane(c, L, &how, j0, tagLen, aData, aDataLen, crtxt, crtxtLen, pntxt);
    }
    DONE(L, rc);
}

int uaes_gcm_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    KEYSCHED(ks);
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    return gcm_decrypt_call(&ks, key, keybits, 1, nonce, nonceLen, tagLen, aData, aDataLen, crtxt, crtxtLen, pntxt);
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

/* ------------------------------------------------------------------------ */
/* XAES-256-GCM (C2SP): AES-256-GCM under a key made of half a 24-byte nonce   */
/* ------------------------------------------------------------------------ */
/* CMAC's first subkey under the master key: K1 = 2 AES_K(0^128) in GF(2^128), big-endian, x^128 = x^7 + x^2 + x + 1.
 * Per call, and secret: the caller burns it (the batches hand it to their kernel, uaes_engine_modes.c). */
void xaes_k1(const keysched *mk, uint8_t k1[16])
{
    static const uint8_t zero[16];
    uint8_t l[16];
    int i;
    uaesh_encrypt(mk->ek.w, mk->nr, zero, l);
    for (i = 0; i < 16; ++i) k1[i] = (uint8_t)((l[i] << 1) | (i < 15 ? l[i + 1] >> 7 : 0));
    k1[15] ^= (uint8_t)(0x87 & -(l[0] >> 7));
    burn(l, sizeof l);
}

/* Kx = CMAC_K(00 01 58 00 || N[0:12]) || CMAC_K(00 02 58 00 || N[0:12]): each message is one whole block, so each MAC
 * is one block of the cipher over message ^ K1.  Three blocks of the host cipher in all; no device is touched. */
static int xaes_derive(const uint8_t *key, const uint8_t *nonce, uint8_t kx[32])
{
    KEYSCHED(mk);
    uint8_t k1[16], m[16];
    int rc, i, half;
    if (!key || !nonce) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&mk, key, 256)) != 0) return rc;
    xaes_k1(&mk, k1);
    for (half = 0; half < 2; ++half) {
        m[0] = 0; m[1] = (uint8_t)(half + 1); m[2] = 0x58; m[3] = 0;
        memcpy(m + 4, nonce, 12);
        for (i = 0; i < 16; ++i) m[i] ^= k1[i];
        uaesh_encrypt(mk.ek.w, mk.nr, m, kx + 16 * half);
    }
    burn(k1, sizeof k1);
    burn(m, sizeof m);
    return 0;
}

int uaes_xaes256gcm_derive(const uint8_t key[32], const uint8_t nonce[24], uint8_t kx[32])
{
    if (!kx) return fail(UAES_E_ARG, "NULL pointer");
    return xaes_derive(key, nonce, kx);
}

/* The one-message calls: Kx on the host, then the one-call GCM path under it with the second half of the nonce -- the
 * fused kernels for a long text, the host data path for a short one where it is switched on, exactly as GCM.  The lane
 * does not remember Kx (cache 0): no later call repeats it. */
static int xaes_call(int decrypt, const uint8_t *key, const uint8_t *nonce, const void *aData, size_t aDataLen,
                     const void *in, size_t len, void *out)
{
    KEYSCHED(ks);
    uint8_t kx[32];
    int rc;
    if ((rc = xaes_derive(key, nonce, kx)) == 0 && (rc = expand_key(&ks, kx, 256)) == 0)
        rc = decrypt ? gcm_decrypt_call(&ks, kx, 256, 0, nonce + 12, 12, 16, aData, aDataLen, in, len, out)
                     : gcm_encrypt_call(&ks, kx, 256, 0, nonce + 12, 12, 16, aData, aDataLen, in, len, out);
    burn(kx, sizeof kx);
    return rc;
}

int uaes_xaes256gcm_encrypt(const uint8_t key[32], const uint8_t nonce[24], const void *aData, size_t aDataLen,
                            const void *pntxt, size_t ptextLen, void *crtxt)
{
    return xaes_call(0, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
}

int uaes_xaes256gcm_decrypt(const uint8_t key[32], const uint8_t nonce[24], const void *aData, size_t aDataLen,
                            const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return xaes_call(1, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
}

/* The *_dev calls: one uaesk_gcm under a 12-byte nonce on the caller's stream, nothing waited for.  slot >= 0: `how`'s
 * scratch is that pinned slot of the context, dropped once the launch is issued. */
static int gcm_call_dev(context *c, const gcm_how *how, int slot, int mode, const uint8_t *nonce,
                        const void *d_aad, size_t aad_len, const void *d_in, size_t len, void *d_out,
                        int *d_status, void *stream)
{
    uint8_t j0[16];
    int k;
    j0_of_nonce12(nonce, j0);
    arm_done_word(how->done_word);
    k = uaesk_gcm(stream, &c->tb, how->ks->nr, &how->ks->ek, mode, j0, d_aad, aad_len, d_in, len, d_out,
                  how->scratch, d_status, how->keyed);
    disarm_done_word_dev(stream, k);
    if (slot >= 0) scratch_unpin(c, slot);
    return k ? fail(UAES_E_HIP, "uaesk_gcm failed: %s", hipGetErrorString((hipError_t)k)) : 0;
}

int uaes_gcm_encrypt_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, size_t aad_len,
                         const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    KEYSCHED(ks);
    void *scr;
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !d_out) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    const gcm_how how = { &ks, 0, scr, scratch_done_word(scr, c->slot[slot].cap) };
    return gcm_call_dev(c, &how, slot, 0, nonce, d_aad, aad_len, d_in, len, d_out, NULL, stream);
}

int uaes_gcm_decrypt_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, size_t aad_len,
                         const void *d_in, size_t len, void *d_out,
                         int *d_status, void *stream)
{
    context *c;
    KEYSCHED(ks);
    void *scr;
    int rc, slot;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !d_in) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if (!d_status) return fail(UAES_E_ARG, "NULL d_status");
    if ((rc = get_context(&c)) != 0) return rc;
    if ((rc = gcm_scratch_locked(c, stream, &scr, &slot)) != 0) return rc;
    const gcm_how how = { &ks, 0, scr, scratch_done_word(scr, c->slot[slot].cap) };
    return gcm_call_dev(c, &how, slot, gcm_decrypt_mode(), nonce, d_aad, aad_len, d_in, len, d_out, d_status, stream);
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
#define KEY_HOW(k)       { &(k)->ks, 1, (k)->scratch, KEY_DONE_WORD(k) }     /* a gcm_how: the calls on the context */

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
        keysched_wipe(&k->ks);
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
        rc = launched("key table", uaesk_gcm_key_tables(L->stream, &c->tb, k->ks.nr, &k->ks.ek, k->scratch));
        if (rc == 0 && hipStreamSynchronize((hipStream_t)L->stream) != hipSuccess) rc = fail(UAES_E_HIP, "key table build failed");
    }
    if (rc) {
        if (k->scratch) (void)hipFree(k->scratch);
        keysched_wipe(&k->ks);
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
    keysched_wipe(&k->ks);
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
    uint8_t j0[16];
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    const gcm_how how = KEY_HOW(k);
    j0_of_nonce12(nonce, j0);
    DONE(L, gcm_encrypt_on_lane(c, L, &how, j0, 16, aData, aDataLen, pntxt, ptextLen, crtxt));
}

int uaes_gcm_key_decrypt(uaes_gcm_key *k, const uint8_t *nonce, const void *aData, size_t aDataLen,
                         const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    uint8_t j0[16];
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !crtxt || (crtxtLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    const gcm_how how = KEY_HOW(k);
    j0_of_nonce12(nonce, j0);
    DONE(L, gcm_decrypt_on_lane(c, L, &how, j0, 16, aData, aDataLen, crtxt, crtxtLen, pntxt));
}

int uaes_gcm_key_encrypt_dev(uaes_gcm_key *k, const uint8_t *nonce, const void *d_aad, size_t aad_len,
                             const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !d_out) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    const gcm_how how = KEY_HOW(k);
    return gcm_call_dev(c, &how, -1, 0, nonce, d_aad, aad_len, d_in, len, d_out, NULL, stream);
}

int uaes_gcm_key_decrypt_dev(uaes_gcm_key *k, const uint8_t *nonce, const void *d_aad, size_t aad_len,
                             const void *d_in, size_t len, void *d_out, int *d_status, void *stream)
{
    context *c;
    int rc;
    if ((rc = key_device_ok(k)) != 0) return rc;
    if (!nonce || !d_in || !d_status) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = dev_ptrs_ok(d_in, d_out, len)) != 0) return rc;
    if ((rc = get_context(&c)) != 0) return rc;
    const gcm_how how = KEY_HOW(k);
    return gcm_call_dev(c, &how, -1, gcm_decrypt_mode(), nonce, d_aad, aad_len, d_in, len, d_out, d_status, stream);
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
    /* uaesk_gcm_record_max(aad_len) is 0 both when only empty records fit and when the AAD alone is too long, so count
     * the GHASH positions -- AAD blocks, text blocks, the length block -- against those of the longest record there is */
    if ((aad_len + 15) / 16 + (rec_len + 15) / 16 + 1 > uaesk_gcm_record_max(0) / 16 + 1)
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
    if (!nrec) return 0;                                      /* no records: no pointer is looked at */
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
    if (nrec && !d_status) return fail(UAES_E_ARG, "NULL d_status");
    if ((rc = records_args_ok(nrec, d_nonces, d_aad, aad_len, d_in, rec_len, in_stride, rec_len + 16,
                              d_out, out_stride, rec_len)) != 0) return rc;
    if (!nrec) {                                              /* no records: nothing failed, no other pointer is looked at */
        if (d_status) HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int), (hipStream_t)stream));
        return 0;
    }
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
            /* variable-length records: whole slots are copied back (below), and the last slot's sixteen bytes behind
             * max_len were not staged -- a last record shorter than max_len leaves them as an earlier call left them */
            if (lens && hipMemsetAsync(d_out + in_span, 0, out_span - in_span, st) != hipSuccess) { rc = fail(UAES_E_HIP, "memset failed"); break; }
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
            if ((rc = launched("gcm records", kk)) != 0) break;
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
 * whose slots were zeroed before the launch, so the tail of a slot reads as zeros (in place: as the caller's own
 * bytes, and zeros where the last slot was not staged). */
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
    KEYSCHED(ks);
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
    KEYSCHED(ks);
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
        if ((rc = launched("ghash", k)) != 0) break;
        rc = lane_fetch(L, gh, L->d_status + 4, 16);
    } while (0);
    DONE(L, rc);
}

/* ------------------------------------------------------------------------ */
/* GCM-SIV (RFC 8452; micro_aes.c:1418-1516)          */
/* ------------------------------------------------------------------------ */
/* Host orchestration only: the host expands the MASTER key and enqueues; key derivation, the derived key's
 * expansion, POLYVAL, the tag and the LE32 counter stream run in kernels and their per-nonce values never leave the
 * device (k_siv_small for a short message, uaesk_gcmsiv_long otherwise).                                       */
static int gcmsiv_on_lane(context *c, lane *L, const keysched *mk, int decrypt, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, const void *in, size_t len, void *out)
{
    io_plan io;
    const void *d_aad;
    int *const d_status = decrypt ? L->d_status : NULL;
    int rc, k, status = -1;
    if ((rc = gcm_scratch(L, SCRATCH_OTHER)) != 0) return rc;
    if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) return rc;
    if ((rc = plan_io(L, in, len + (decrypt ? 16 : 0), out, len + (decrypt ? 0 : 16), &io)) != 0) return rc;
    /* a short message is ONE launch (k_siv_small): key derivation, POLYVAL, tag and keystream in one workgroup; the
     * host only expands the master key (< 0: too long for it) */
    k = uaesk_gcmsiv_small(L->stream, &c->tb, mk->nr, &mk->ek, decrypt, nonce, d_aad, aDataLen, io.din, len, io.dout, d_status);
    if (k < 0) {
        /* a longer one: six or seven launches one behind the other, the per-nonce key, the hash, the tag and the
         * counter made of it stay on the device (uaesk_gcmsiv_long) -- the host waits once.  Decryption is like the
         * reference's: decrypt with the RECEIVED tag as counter, then authenticate (:1500-1502) */
        arm_done_word(scratch_done_word(L->scratch, L->scratch_cap));
        k = uaesk_gcmsiv_long(L->stream, &c->tb, mk->nr, &mk->ek, decrypt, nonce, d_aad, aDataLen, io.din, len, io.dout,
                              L->scratch, d_status);
        arm_done_word(NULL);
    }
    if ((rc = launched("gcm-siv", k)) != 0) return rc;
    if (!decrypt) return finish_io(&io, len + 16);
    /* the text stays (SABOTAGE is a no-op) unless uaes_set_wipe_on_auth_failure(1) */
    if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) return rc;
    io.drained = 1;
    if ((rc = status ? finish_io_unauthenticated(&io, len) : finish_io(&io, len)) != 0) return rc;
    return status ? UAES_E_AUTHENTICATION : 0;
}

int uaes_gcmsiv_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt)
{
    context *c;
    lane *L;
    KEYSCHED(mk);
    int rc;
    if (keybits != 128 && keybits != 192 && keybits != 256)
        return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if (!key || !nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if ((rc = expand_key(&mk, key, keybits)) != 0) return rc;       /* (checked above: it cannot fail) */
    if (host_take(pntxt, crtxt, ptextLen, 0) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&mk);
        rc = uaesh_gcmsiv(&hk, keybits, 0, nonce, (const uint8_t *)aData, aDataLen, (const uint8_t *)pntxt, ptextLen, (uint8_t *)crtxt, uaes_expand_key);
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    DONE(L, gcmsiv_on_lane(c, L, &mk, 0, nonce, aData, aDataLen, pntxt, ptextLen, crtxt));
}

int uaes_gcmsiv_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt)
{
    context *c;
    lane *L;
    KEYSCHED(mk);
    int rc;
    if (keybits != 128 && keybits != 192 && keybits != 256)
        return fail(UAES_E_ARG, "keybits must be 128, 192 or 256 (got %d)", keybits);
    if (!key || !nonce || !crtxt || (crtxtLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if ((rc = expand_key(&mk, key, keybits)) != 0) return rc;       /* (checked above: it cannot fail) */
    if (host_take(crtxt, pntxt, crtxtLen, 0) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&mk);
        rc = uaesh_gcmsiv(&hk, keybits, 1, nonce, (const uint8_t *)aData, aDataLen, (const uint8_t *)crtxt, crtxtLen, (uint8_t *)pntxt, uaes_expand_key);
        if (rc == UAES_E_AUTHENTICATION && wipe_on_auth_failure()) memset(pntxt, 0, crtxtLen);
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    DONE(L, gcmsiv_on_lane(c, L, &mk, 1, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt));
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
    if ((rc = expand_key(&s->ks, key, keybits)) != 0 || (rc = enter(&c, &L)) != 0) { keysched_wipe(&s->ks); free(s); return rc; }
    memcpy(s->nonce, nonce, 12);
    s->decrypt = decrypt != 0;
    s->aad_len = aDataLen;
    pthread_mutex_lock(&c->mu);
    if (c->nspool > 0) s->scratch = c->spool[--c->nspool];
    pthread_mutex_unlock(&c->mu);
    if (hipGetDevice(&s->device) != hipSuccess ||
        (!s->scratch && hipMalloc(&s->scratch, STREAM_SCRATCH_BYTES + 64) != hipSuccess)) {
        keysched_wipe(&s->ks);
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
        if ((rc = launched("gcm stream", k)) != 0) break;
        rc = lane_sync(L);
    } while (0);
    if (rc) { (void)lane_abandon(L, rc); (void)hipFree(s->scratch); keysched_wipe(&s->ks); free(s); return rc; }
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
        if (k != 1 && (rc = launched("gcm stream", k)) != 0) break;
        if (s->decrypt) {                             /* hash the ciphertext before it may be overwritten */
            k = uaesk_gcm_stream_absorb(L->stream, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, 1, io.din, len, 0, 0, s->scratch, &s->plan_state);
            if (!k) k = uaesk_ctr_xcrypt(L->stream, &c->tb, s->ks.nr, &s->ks.ek, &ctr, io.din, io.dout, len, NULL);
        } else {
            k = uaesk_ctr_xcrypt(L->stream, &c->tb, s->ks.nr, &s->ks.ek, &ctr, io.din, io.dout, len, NULL);
            if (!k) k = uaesk_gcm_stream_absorb(L->stream, &c->tb, s->ks.nr, &s->ks.ek, s->nonce, 1, io.dout, len, 0, 0, s->scratch, &s->plan_state);
        }
        if ((rc = launched("gcm stream", k)) != 0) break;
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

/* test hook (include/uaes_hip.h): which GHASH tables the stream's scratch holds */
unsigned uaes_debug_gcm_stream_tables(const uaes_gcm_stream *s) { return s ? s->plan_state : 0u; }

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
    keysched_wipe(&s->ks);
    free(s);
}

/* ------------------------------------------------------------------------ */
/* one shard of a GCM message (uaes_engine_mgpu.c: GCM over several GPUs)      */
/* ------------------------------------------------------------------------ */
/* One shard of a GCM message on the calling thread's current device, synchronously: the CTR pass (mode 0 / 2) fused
 * with the shard's weighted share of Enc(J0) ^ GHASH (uaesk_gcm_shard); mode 1 hashes only.  in / out host or device. */
int gcm_shard_sync(int keybits, const uint8_t *key, const uint8_t *nonce, int mode,
                   const void *aData, uint64_t aDataLen, const void *in, size_t len, uint64_t off,
                   uint64_t total, void *out, uint8_t share[16])
{
    context *c;
    lane *L;
    KEYSCHED(ks);
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
        if ((rc = launched("gcm shard", k)) != 0) break;
        if ((rc = lane_fetch(L, share, L->d_status + 4, 16)) != 0) break;
        if (mode != 1) { io.drained = 1; rc = finish_io(&io, len); }
    } while (0);
    DONE(L, rc);
}
