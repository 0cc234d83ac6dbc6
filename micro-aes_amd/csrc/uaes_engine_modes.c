/*
 * uaes_engine_modes.c -- entry points of the modes other than GCM: ECB, CTR, XTS, CMAC, Poly1305, CCM, EAX, EAX', SIV,
 * CBC / CFB / OFB, the chain batches, OCB, key wrap (KW and KWP), FF1 and FF3-1.  They mirror the reference's mode
 * drivers (AES_ECB_*, AES_CTR_*, AES_XTS_* ...; micro_aes.c:636-680, :962-990, :1066-1093): argument checking, the
 * reference's error behaviour and buffer plumbing on top of the core (uaes_engine.c, through uaes_engine.h).
 */
#include "uaes_engine.h"

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
    KEYSCHED(ks);
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
        if (!decrypt) { uaesh_ecb_encrypt(&hk, padding, (const uint8_t *)in, len, (uint8_t *)out); return host_result(0); }
        uaesh_ecb_decrypt(&hk, (const uint8_t *)in, len, (uint8_t *)out);
        return host_result(rem ? UAES_E_DECRYPTION : 0);
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
        if ((rc = launched("ecb", k)) != 0) break;
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
    KEYSCHED(ks);
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
int uaes_ctr_xcrypt_at_dev(int keybits, const uint8_t *key, const uint8_t ctr0[16],
                           uint64_t block_offset,
                           const void *d_in, size_t len, void *d_out, void *stream)
{
    context *c;
    KEYSCHED(ks);
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
    KEYSCHED(ks);
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
        return host_result(0);
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
        if ((rc = launched("ctr", k)) != 0) break;
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
    return launched("xts", k);
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
    KEYSCHED(k1);
    KEYSCHED(k2);
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
        return host_result(0);
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
    KEYSCHED(k1);
    KEYSCHED(k2);
    int rc;
    if ((rc = xts_keys(&k1, &k2, keys, keybits)) != 0) return rc;
    if ((rc = dev_ptrs_ok(d_in, d_out, sector_bytes * nsectors)) != 0) return rc;
    if (sector_bytes < 16) return UAES_E_DATALENGTH;
    if ((rc = get_context(&c)) != 0) return rc;
    return xts_run(c, stream, &k1, &k2, encrypt, NULL, first_sector, sector_bytes, nsectors, d_in, d_out, NULL);
}

/* Batches of data units, sixteen GPU lanes per unit (k_xts_batch, uaes_xts_batch.hip): nmsg units in slots of msg_bytes,
 * one launch, always on the GPU.  tweaks = tweak_bytes per unit: 16 raw bytes, or 8, a sector number (the kernel
 * widens it to LE128).  The conventions are the cipher batches' (cipher_rows): every array host or device memory at any
 * byte offset, host arrays through the lane's scratch and staging buffers; with `lens` a host-memory output starts as a
 * copy of the caller's buffer and the status word is armed, which a unit below 16 bytes sets.  The order: the sizes,
 * the keys, nothing more for no units, a slot below 16 bytes, the pointers, and only then the device. */
static int xts_rows(int encrypt, int keybits, const uint8_t *keys, const void *tweaks, unsigned tweak_bytes, size_t nmsg,
                    size_t msg_bytes, const uint32_t *lens, const void *in, void *outp)
{
    const size_t total = nmsg * msg_bytes;
    context *c;
    lane *L;
    KEYSCHED(k1);
    KEYSCHED(k2);
    int rc, k, bad;
    if (msg_bytes > UINT32_MAX)
        return fail(UAES_E_ARG, "a batch unit holds at most %u bytes (got %zu)", UINT32_MAX, msg_bytes);
    if (nmsg > (size_t)-1 / 2 / (msg_bytes > 16 ? msg_bytes : 16))     /* / 2: the tweaks, the lengths and their padding */
        return fail(UAES_E_ARG, "batch size overflows");
    if ((rc = xts_keys(&k1, &k2, keys, keybits)) != 0) return rc;
    if (nmsg == 0) return 0;
    if (msg_bytes < 16) return UAES_E_DATALENGTH;                /* :1069, untouched */
    if (!tweaks || !in || !outp) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    row_array a[2] = { { tweaks, nmsg * tweak_bytes, 0, NULL }, { lens, lens ? nmsg * sizeof *lens : 0, 0, NULL } };
    row_text t = { in, outp, total, total, lens != NULL, NULL, NULL };
    if (lens && is_device_ptr(lens) && ((uintptr_t)lens & 3u)) {
        rc = fail(UAES_E_ARG, "a device array of lengths must be 4-byte aligned");
        goto out;
    }
    if ((rc = row_stage(L, a, 2, lens != NULL)) != 0) goto out;
    if ((rc = row_texts(L, &t)) != 0) goto out;
    k = uaesk_xts_batch(L->stream, &c->tb, k1.nr, encrypt ? &k1.ek : &k1.dk, &k2.ek, !encrypt, a[0].d, tweak_bytes, nmsg,
                        msg_bytes, a[1].d, t.d_in, t.d_out, L->d_status);
    if ((rc = launched("xts batch", k)) != 0) goto out;
    if ((rc = row_finish(L, &t, a, 2, lens != NULL, &bad)) != 0) goto out;
    if (bad) rc = UAES_E_DATALENGTH;
out:
    DONE(L, rc);
}

int uaes_xts_encrypt_batch(int keybits, const uint8_t *keys, const uint8_t *tweaks, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *pntxt, void *crtxt)
{
    return xts_rows(1, keybits, keys, tweaks, 16, nmsg, msg_bytes, lens, pntxt, crtxt);
}

int uaes_xts_decrypt_batch(int keybits, const uint8_t *keys, const uint8_t *tweaks, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *crtxt, void *pntxt)
{
    return xts_rows(0, keybits, keys, tweaks, 16, nmsg, msg_bytes, lens, crtxt, pntxt);
}

int uaes_xts_sector_list(int keybits, const uint8_t *keys, const uint64_t *sectors, size_t nsectors,
                         size_t sector_bytes, const void *in, void *out, int encrypt)
{
    return xts_rows(encrypt != 0, keybits, keys, sectors, 8, nsectors, sector_bytes, NULL, in, out);
}

/* ------------------------------------------------------------------------ */
/* CMAC and CCM: serial CBC-MAC chains, one GPU lane */
/* ------------------------------------------------------------------------ */
int uaes_cmac(int keybits, const uint8_t *key, const void *data, size_t dataSize, uint8_t mac[16])
{
    context *c;
    lane *L;
    KEYSCHED(ks);
    io_plan io;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!mac || (dataSize && !data)) return fail(UAES_E_ARG, "NULL pointer");
    if (host_take(data, NULL, dataSize, 1)) {
        const uaesh_key hk = host_key(&ks);
        uaesh_cmac(&hk, (const uint8_t *)data, dataSize, mac);
        return host_result(0);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = plan_io(L, data, dataSize, NULL, 0, &io)) != 0) break;
        int k = uaesk_cmac(L->stream, &c->tb, ks.nr, &ks.ek, io.din, dataSize, L->d_status + 4);
        if ((rc = launched("cmac", k)) != 0) break;
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
    KEYSCHED(ks);
    io_plan io;
    int rc;
    if (!keys || !nonce || !mac || (dataSize && !data)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&ks, keys, keybits)) != 0) return rc;
    const uint8_t *r = keys + keybits / 8;
    if (host_take(data, NULL, dataSize, 0)) {
        const uaesh_key hk = host_key(&ks);
        uaesh_poly1305(&hk, r, nonce, (const uint8_t *)data, dataSize, mac);
        return host_result(0);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        const size_t need = uaesk_poly1305_scratch_bytes(dataSize);
        if ((rc = plan_io(L, data, dataSize, NULL, 0, &io)) != 0) break;
        if (need && (rc = lane_scratch(L, need, SCRATCH_OTHER)) != 0) break;
        int k = uaesk_poly1305(L->stream, &c->tb, ks.nr, &ks.ek, r, nonce, io.din, dataSize, L->d_status + 4,
                               need ? L->scratch : NULL);
        if ((rc = launched("poly1305", k)) != 0) break;
        rc = lane_fetch(L, mac, L->d_status + 4, 16);
    } while (0);
    DONE(L, rc);
}

int uaes_poly1305_dev(int keybits, const uint8_t *keys, const uint8_t nonce[16],
                      const void *d_data, size_t len, void *d_mac, void *stream)
{
    context *c;
    KEYSCHED(ks);
    void *scr = NULL;
    int rc, slot = -1;
    if (!keys || !nonce || !d_mac || (len && !d_data)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&ks, keys, keybits)) != 0) return rc;
    const size_t need = uaesk_poly1305_scratch_bytes(len);
    if ((rc = get_context(&c)) != 0) return rc;
    if (need) {
        pthread_mutex_lock(&c->mu);
        rc = scratch_pin(c, stream, need, &scr, &slot);
        pthread_mutex_unlock(&c->mu);
        if (rc) return fail(UAES_E_HIP, "poly1305 scratch");
    }
    rc = uaesk_poly1305(stream, &c->tb, ks.nr, &ks.ek, keys + keybits / 8, nonce, d_data, len, d_mac, scr);
    KCHK_PINNED(c, slot, rc);
    return 0;
}

int uaes_poly1305_batch(int keybits, const uint8_t *keys, const uint8_t *nonces, size_t nmsg,
                        size_t msg_bytes, const void *data, uint8_t *macs)
{
    context *c;
    lane *L;
    KEYSCHED(ks);
    io_plan io;
    const void *d_nonces = NULL;
    int rc;
    if (msg_bytes && nmsg > (size_t)-1 / msg_bytes) return fail(UAES_E_ARG, "batch size overflows");
    if (!keys || (nmsg && (!nonces || !macs)) || (nmsg && msg_bytes && !data)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = expand_key(&ks, keys, keybits)) != 0) return rc;
    if (nmsg == 0) return 0;
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = stage_aad(L, nonces, nmsg * 16, &d_nonces)) != 0) break;       /* host nonces -> device */
        if ((rc = plan_io(L, data, nmsg * msg_bytes, macs, nmsg * 16, &io)) != 0) break;
        if (io.dout == io.din && io.copy_back) {                  /* MACs must not overwrite unread messages */
            if (grow_on(L->stream, &L->stage[1], &L->stage_cap[1], nmsg * 16 + 64)) { rc = UAES_E_HIP; break; }
            io.dout = L->stage[1];
        }
        int k = uaesk_poly1305_batch(L->stream, &c->tb, ks.nr, &ks.ek, keys + keybits / 8, d_nonces, nmsg, msg_bytes,
                                     io.din, io.dout);
        if ((rc = launched("poly1305 batch", k)) != 0) break;
        rc = finish_io(&io, nmsg * 16);
    } while (0);
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
    KEYSCHED(ks);
    io_plan io;
    const void *d_aad;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!nonce || !crtxt || (ptextLen && !pntxt)) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = ccm_lens_ok(nonceLen, tagLen)) != 0) return rc;
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(pntxt, crtxt, ptextLen, 1) && !is_device_ptr(aData)) {
        const uaesh_key hk = host_key(&ks);
        return host_result(uaesh_ccm(&hk, 0, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen, (const uint8_t *)pntxt, ptextLen, (uint8_t *)crtxt));
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, pntxt, ptextLen, crtxt, ptextLen + tagLen, &io)) != 0) break;
        int k = uaesk_ccm(L->stream, &c->tb, ks.nr, &ks.ek, 0, nonce, nonceLen, tagLen, d_aad, aDataLen,
                          io.din, ptextLen, io.dout, NULL);
        if ((rc = launched("ccm", k)) != 0) break;
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
    KEYSCHED(ks);
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
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = stage_aad(L, aData, aDataLen, &d_aad)) != 0) break;
        if ((rc = plan_io(L, crtxt, crtxtLen + tagLen, pntxt, crtxtLen, &io)) != 0) break;
        int k = uaesk_ccm(L->stream, &c->tb, ks.nr, &ks.ek, 1, nonce, nonceLen, tagLen, d_aad, aDataLen,
                          io.din, crtxtLen, io.dout, L->d_status);
        if ((rc = launched("ccm", k)) != 0) break;
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

static int eax_common(int keybits, const uint8_t *key, int decrypt, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                      const void *aData, size_t aDataLen, const void *in, size_t len, void *outp)
{
    context *c;
    lane *L;
    KEYSCHED(ks);
    io_plan io;
    const void *d_nonce, *d_aad;
    size_t off = 0;
    int rc, k, status = 0;
    uint8_t res[32];
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!in || (len && !outp) || (nonceLen && !nonce)) return fail(UAES_E_ARG, "NULL pointer");
    if (!decrypt && !outp) return fail(UAES_E_ARG, "NULL pointer");
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "EAX tag length %zu (1..16)", tagLen);
    if (aDataLen && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (host_take(in, outp, len, 1) && !is_device_ptr(aData) && !is_device_ptr(nonce)) {
        const uaesh_key hk = host_key(&ks);
        return host_result(uaesh_eax(&hk, decrypt, nonce, nonceLen, tagLen, (const uint8_t *)aData, aDataLen,
                                     (const uint8_t *)in, len, (uint8_t *)outp));
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
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
            k = uaesk_eax_small(L->stream, &c->tb, ks.nr, &ks.ek, decrypt, d_nonce, nonceLen, d_aad, aDataLen,
                                io.din, len, io.dout, tag, tl, decrypt ? L->d_status : NULL);
            if ((rc = launched("eax", k)) != 0) goto out;
            if (decrypt) {
                if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) goto out;
                io.drained = 1;
            }
        } else {                                          /* eax.long: the chains, one fetch, then CTR */
            uaesk_ctr ctr;
            k = uaesk_eax_macs(L->stream, &c->tb, ks.nr, &ks.ek, decrypt ? 1 : 0, d_nonce, nonceLen,
                               d_aad, aDataLen, decrypt ? io.din : NULL, decrypt ? len : 0, tag, tl, L->d_status);
            if ((rc = launched("eax", k)) != 0) goto out;
            if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
            memcpy(&status, res, sizeof status);
            if (decrypt && status) {
                io.drained = 1;
            } else {
                make_ctr(&ctr, res + 16, 0);
                k = uaesk_ctr_xcrypt(L->stream, &c->tb, ks.nr, &ks.ek, &ctr, io.din, io.dout, len, NULL);
                if ((rc = launched("eax ctr", k)) != 0) goto out;
                if (!decrypt) {
                    k = uaesk_eax_macs(L->stream, &c->tb, ks.nr, &ks.ek, 2, NULL, 0, NULL, 0, io.dout, len, tag, tl, L->d_status);
                    if ((rc = launched("eax", k)) != 0) goto out;
                }
            }
        }
    }
    /* the tag is checked before anything is written (:1638-1645): a forgery leaves pntxt as it was */
    if (decrypt && status) rc = UAES_E_AUTHENTICATION;
    else rc = finish_io(&io, decrypt ? len : len + tagLen);
out:
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

/* EAX' (the reference built with EAXP 1, :1523-1648): eax_common's shape without associated data and with the 4-byte mac
 * behind the text; the kernels hand back N' as the counter block (k_eaxp_small / k_eaxp_macs, uaes_eax_siv.hip) */
static int eaxp_common(int keybits, const uint8_t *key, int decrypt, const uint8_t *nonce, size_t nonceLen,
                       const void *in, size_t len, void *outp)
{
    context *c;
    lane *L;
    KEYSCHED(ks);
    io_plan io;
    const void *d_nonce;
    size_t off = 0;
    int rc, k, status = 0;
    uint8_t res[32];
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (!in || (len && !outp) || (nonceLen && !nonce)) return fail(UAES_E_ARG, "NULL pointer");
    if (!decrypt && !outp) return fail(UAES_E_ARG, "NULL pointer");
    if (len > (size_t)-1 - 64) return fail(UAES_E_ARG, "the text length overflows");
    if (host_take(in, outp, len, 1) && !is_device_ptr(nonce)) {
        const uaesh_key hk = host_key(&ks);
        return host_result(uaesh_eaxp(&hk, decrypt, nonce, nonceLen, (const uint8_t *)in, len, (uint8_t *)outp));
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    if ((rc = lane_scratch(L, SIDE(nonceLen), SCRATCH_OTHER)) != 0) goto out;
    if ((rc = side_in(L, &off, nonce, nonceLen, &d_nonce)) != 0) goto out;
    if (decrypt) rc = plan_io(L, in, len + 4, outp, len, &io);
    else rc = plan_io(L, in, len, outp, len + 4, &io);
    if (rc) goto out;
    {
        unsigned char *mac = decrypt ? (unsigned char *)io.din + len : (unsigned char *)io.dout + len;
        if (len <= UAES_EAX_SIV_SMALL_MAX) {             /* eaxp.small: one launch */
            k = uaesk_eaxp_small(L->stream, &c->tb, ks.nr, &ks.ek, decrypt, d_nonce, nonceLen, io.din, len, io.dout, mac,
                                 decrypt ? L->d_status : NULL);
            if ((rc = launched("eax'", k)) != 0) goto out;
            if (decrypt) {
                if ((rc = lane_fetch(L, &status, L->d_status, sizeof status)) != 0) goto out;
                io.drained = 1;
            }
        } else {                                          /* eaxp.long: the chains, one fetch, then CTR */
            uaesk_ctr ctr;
            k = uaesk_eaxp_macs(L->stream, &c->tb, ks.nr, &ks.ek, decrypt ? 1 : 0, d_nonce, nonceLen, decrypt ? io.din : NULL,
                                decrypt ? len : 0, mac, L->d_status);
            if ((rc = launched("eax'", k)) != 0) goto out;
            if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
            memcpy(&status, res, sizeof status);
            if (decrypt && status) {
                io.drained = 1;
            } else {
                make_ctr(&ctr, res + 16, 0);
                k = uaesk_ctr_xcrypt(L->stream, &c->tb, ks.nr, &ks.ek, &ctr, io.din, io.dout, len, NULL);
                if ((rc = launched("eax' ctr", k)) != 0) goto out;
                if (!decrypt) {
                    k = uaesk_eaxp_macs(L->stream, &c->tb, ks.nr, &ks.ek, 2, NULL, 0, io.dout, len, mac, L->d_status);
                    if ((rc = launched("eax'", k)) != 0) goto out;
                }
            }
        }
    }
    /* the mac is checked before anything is written (:1631-1643): a forgery leaves pntxt as it was */
    if (decrypt && status) rc = UAES_E_AUTHENTICATION;
    else rc = finish_io(&io, decrypt ? len : len + 4);
out:
    memset(res, 0, sizeof res);
    DONE(L, rc);
}

int uaes_eaxp_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                      const void *pntxt, size_t ptextLen, void *crtxt)
{
    if (!pntxt && !ptextLen) pntxt = crtxt;                       /* (nothing is read) */
    return eaxp_common(keybits, key, 0, nonce, nonceLen, pntxt, ptextLen, crtxt);
}

int uaes_eaxp_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                      const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return eaxp_common(keybits, key, 1, nonce, nonceLen, crtxt, crtxtLen, pntxt);
}

static int siv_keys(keysched *k1, keysched *k2, const uint8_t *keys, int keybits)
{
    int rc;
    if (!keys) return fail(UAES_E_ARG, "NULL keys");
    if ((rc = expand_key(k1, keys, keybits)) != 0) return rc;
    return expand_key(k2, keys + keybits / 8, keybits);
}

typedef char uaes_siv_ad_limits_are_the_kernels[UAES_SIV_AD_MAX == UAES_S2V_AD_MAX && UAES_SIV_BATCH_AD_MAX == UAES_S2V_BATCH_AD_MAX ? 1 : -1];

/* the components of SIV's associated data: at most `most` of them, their lengths, the bytes they add up to */
static int siv_components(size_t nad, const size_t *adLens, size_t most, size_t *total)
{
    size_t i;
    *total = 0;
    if (nad > most) return fail(UAES_E_ARG, "S2V takes at most %zu components here (got %zu)", most, nad);
    if (nad && !adLens) return fail(UAES_E_ARG, "NULL adLens with nad != 0");
    for (i = 0; i < nad; ++i) {
        if (adLens[i] > (size_t)-1 - 64 - *total) return fail(UAES_E_ARG, "the component lengths overflow");
        *total += adLens[i];
    }
    return 0;
}

/* aData = nad components back to back.  vec: the _v calls, whose kernels (k_s2v_v) deal the components over the
 * workgroup's rows and get the running totals of the lengths through the scratch, behind the components; else the
 * one-aData calls and their kernels, nad = 0 or 1. */
static int siv_common(int keybits, const uint8_t *keys, int decrypt, uint8_t *iv, int vec, size_t nad, const size_t *adLens,
                      const void *aData, const void *in, size_t len, void *outp)
{
    context *c;
    lane *L;
    KEYSCHED(k1);
    KEYSCHED(k2);
    io_plan io;
    const void *d_aad, *d_ends = NULL;
    size_t off = 0, total, i;
    int rc, k, status = 0;
    uint8_t v[16], res[32];
    uint64_t ends[UAES_SIV_AD_MAX];
    if ((rc = siv_components(nad, adLens, UAES_SIV_AD_MAX, &total)) != 0) return rc;
    if ((rc = siv_keys(&k1, &k2, keys, keybits)) != 0) return rc;
    if (!iv || (len && (!in || !outp))) return fail(UAES_E_ARG, "NULL pointer");
    if (total && !aData) return fail(UAES_E_ARG, "NULL aData with aDataLen != 0");
    if (decrypt && (rc = iv_read(v, iv)) != 0) return rc;
    if (host_take(in, outp, len, 1) && !is_device_ptr(aData) && !is_device_ptr(iv)) {
        const uaesh_key h1 = host_key(&k1), h2 = host_key(&k2);
        rc = uaesh_siv(&h1, &h2, decrypt, v, nad, adLens, (const uint8_t *)aData, (const uint8_t *)in, len, (uint8_t *)outp);
        if (!decrypt) memcpy(iv, v, 16);
        if (rc && len && wipe_on_auth_failure()) memset(outp, 0, len);       /* (the default leaves the text, as the reference does) */
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    if ((rc = lane_scratch(L, SIDE(total) + (vec ? SIDE(nad * sizeof *ends) : 0), SCRATCH_OTHER)) != 0) goto out;
    if ((rc = side_in(L, &off, aData, total, &d_aad)) != 0) goto out;
    if (vec) {
        for (i = 0; i < nad; ++i) ends[i] = (i ? ends[i - 1] : 0) + adLens[i];
        if ((rc = side_in(L, &off, ends, nad * sizeof *ends, &d_ends)) != 0) goto out;
    }
    if ((rc = plan_io(L, len ? in : NULL, len, len ? outp : NULL, len, &io)) != 0) goto out;
    if (len <= UAES_EAX_SIV_SMALL_MAX) {                  /* s2v.small: one launch */
        k = vec ? uaesk_s2v_v(L->stream, &c->tb, k1.nr, &k1.ek, &k2.ek, decrypt, 1, decrypt ? v : NULL, d_aad, d_ends, (unsigned)nad,
                              io.din, len, io.dout, L->d_status)
                : uaesk_s2v_small(L->stream, &c->tb, k1.nr, &k1.ek, &k2.ek, decrypt, decrypt ? v : NULL, d_aad, total,
                                  io.din, len, io.dout, (char *)L->d_status + 16, decrypt ? L->d_status : NULL);
        if ((rc = launched("siv", k)) != 0) goto out;
        if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
        io.drained = 1;
    } else if (!decrypt) {                                /* s2v.long: the chains, one fetch, then CTR(V') */
        uaesk_ctr ctr;
        k = vec ? uaesk_s2v_v(L->stream, &c->tb, k1.nr, &k1.ek, &k2.ek, 0, 0, NULL, d_aad, d_ends, (unsigned)nad, io.din, len,
                              io.dout, L->d_status)
                : uaesk_s2v_macs(L->stream, &c->tb, k1.nr, &k1.ek, 0, NULL, d_aad, total, io.din, len, L->d_status);
        if ((rc = launched("siv", k)) != 0) goto out;
        if ((rc = lane_fetch(L, res, L->d_status, sizeof res)) != 0) goto out;
        memcpy(v, res + 16, 16);
        v[8] &= 0x7F;
        v[12] &= 0x7F;
        make_ctr(&ctr, v, 0);
        k = uaesk_ctr_xcrypt(L->stream, &c->tb, k2.nr, &k2.ek, &ctr, io.din, io.dout, len, NULL);
        if ((rc = launched("siv ctr", k)) != 0) goto out;
    } else {                                              /* decrypt: CTR(iv') first, S2V over what it wrote, one fetch */
        uaesk_ctr ctr;
        uint8_t cv[16];
        memcpy(cv, v, 16);
        cv[8] &= 0x7F;
        cv[12] &= 0x7F;
        make_ctr(&ctr, cv, 0);
        k = uaesk_ctr_xcrypt(L->stream, &c->tb, k2.nr, &k2.ek, &ctr, io.din, io.dout, len, NULL);
        if ((rc = launched("siv ctr", k)) != 0) goto out;
        k = vec ? uaesk_s2v_v(L->stream, &c->tb, k1.nr, &k1.ek, &k2.ek, 1, 0, v, d_aad, d_ends, (unsigned)nad, io.din, len,
                              io.dout, L->d_status)
                : uaesk_s2v_macs(L->stream, &c->tb, k1.nr, &k1.ek, 1, v, d_aad, total, io.dout, len, L->d_status);
        if ((rc = launched("siv", k)) != 0) goto out;
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
    DONE(L, rc);
}

/* the one-aData calls: an empty AAD is no header unit (micro_aes.c:1333-1344), so it is no component */
int uaes_siv_encrypt(int keybits, const uint8_t *keys, const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, uint8_t iv[16], void *crtxt)
{
    return siv_common(keybits, keys, 0, iv, 0, aDataLen ? 1 : 0, &aDataLen, aData, pntxt, ptextLen, crtxt);
}

int uaes_siv_decrypt(int keybits, const uint8_t *keys, const uint8_t iv[16], const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return siv_common(keybits, keys, 1, (uint8_t *)iv, 0, aDataLen ? 1 : 0, &aDataLen, aData, crtxt, crtxtLen, pntxt);
}

int uaes_siv_encrypt_v(int keybits, const uint8_t *keys, size_t nad, const size_t *adLens, const void *aData,
                       const void *pntxt, size_t ptextLen, uint8_t iv[16], void *crtxt)
{
    return siv_common(keybits, keys, 0, iv, 1, nad, adLens, aData, pntxt, ptextLen, crtxt);
}

int uaes_siv_decrypt_v(int keybits, const uint8_t *keys, const uint8_t iv[16], size_t nad, const size_t *adLens,
                       const void *aData, const void *crtxt, size_t crtxtLen, void *pntxt)
{
    return siv_common(keybits, keys, 1, (uint8_t *)iv, 1, nad, adLens, aData, crtxt, crtxtLen, pntxt);
}

/* ---- AEAD record batches: EAX, EAX', SIV, CCM, GCM-SIV, multi-key GCM, XAES-256-GCM and OCB ----
 * nmsg records of msg_bytes each in one launch, sixteen lanes per record.  Every array may be host or device memory;
 * host arrays travel through the lane's staging buffers and scratch.  A mode checks its own limits, describes the call
 * in an aead_rows and hands it to aead_rows_run, which does everything the modes share, in this order: the sizes, the
 * key, nothing more for no records, the pointers, and only then the device.  What a mode adds is its launch.       */
enum { AB_KEYS, AB_NONCES, AB_NLENS, AB_AAD, AB_LENS, AB_TAGS, AB_VERDICTS, AB_NSIDE };      /* the side arrays, in scratch order (AB_NLENS: EAX' alone) */

typedef struct aead_rows aead_rows;
struct aead_rows {
    const char    *name;                /* of the mode, for a launch that fails */
    int            nkeys, keybits;      /* host key schedules made of `key`: 1, SIV's 2, or 0 (AB_KEYS: the kernel expands them) */
    const uint8_t *key;
    int            decrypt;             /* tags are read and verdicts written, not tags written */
    int            prefill;             /* the kernel leaves records unwritten: the output's staging starts as the caller's
                                         * buffer (row_text).  With AB_LENS it does so whatever this says: the rest of a slot */
    size_t         nmsg, msg_bytes;
    const void    *in;
    void          *out;
    struct { const void *p; size_t each; } side[AB_NSIDE];   /* the caller's arrays and their bytes per record; 0: the
                                                              * call has no such array */
    size_t         nad;                 /* SIV's _v batches: every record's AAD slot is these components */
    const size_t  *ad_lens;
    int          (*launch)(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t);
};

static int aead_rows_staged(const aead_rows *b, const keysched *const ks[2])
{
    context *c;
    lane *L;
    const size_t total = b->nmsg * b->msg_bytes;
    row_array a[AB_NSIDE];
    row_text t = { b->in, b->out, total, total, b->prefill || b->side[AB_LENS].each, NULL, NULL };
    int i, rc, bad;
    if (total && (!b->in || !b->out)) return fail(UAES_E_ARG, "NULL pointer");
    for (i = 0; i < AB_NSIDE; ++i) {
        if (b->side[i].each && !b->side[i].p) return fail(UAES_E_ARG, "NULL pointer");
        a[i] = (row_array){ b->side[i].p, b->nmsg * b->side[i].each, i == AB_VERDICTS || (i == AB_TAGS && !b->decrypt), NULL };
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    if ((rc = row_stage(L, a, AB_NSIDE, b->decrypt)) == 0 && (rc = row_texts(L, &t)) == 0)
        rc = launched(b->name, b->launch(b, c, L, ks, a, &t));
    if (b->side[AB_KEYS].each) {
        /* keys in host memory went through the scratch: that copy is cleared in stream order before the call returns,
         * however far it got (a failure to clear is reported if nothing failed before), and an error waits for it */
        if (a[AB_KEYS].d && a[AB_KEYS].d != b->side[AB_KEYS].p &&
            hipMemsetAsync(a[AB_KEYS].d, 0, a[AB_KEYS].bytes, (hipStream_t)L->stream) != hipSuccess && rc == 0)
            rc = fail(UAES_E_HIP, "clearing the staged keys failed");
        if (rc) (void)hipStreamSynchronize((hipStream_t)L->stream);
    }
    if (rc == 0 && (rc = row_finish(L, &t, a, AB_NSIDE, b->decrypt, &bad)) == 0 && bad) rc = UAES_E_AUTHENTICATION;
    DONE(L, rc);
}

static int aead_rows_run(const aead_rows *b)
{
    KEYSCHED(k1);
    KEYSCHED(k2);
    const keysched *const ks[2] = { &k1, &k2 };
    size_t widest = b->msg_bytes;
    int i, rc;
    for (i = 0; i < AB_NSIDE; ++i)
        if (b->side[i].each > widest) widest = b->side[i].each;
    if (widest && b->nmsg > (size_t)-1 / 8 / widest)     /* / 8: the side arrays and their padding still add up */
        return fail(UAES_E_ARG, "batch size overflows");
    rc = b->nkeys == 2 ? siv_keys(&k1, &k2, b->key, b->keybits) : b->nkeys ? expand_key(&k1, b->key, b->keybits) : 0;
    if (rc == 0 && b->nmsg) rc = aead_rows_staged(b, ks);
    return rc;
}

/* EAX and SIV batches (k_eax_batch, k_s2v_batch: uaes_eax_siv.hip): 16-byte tags; SIV has no nonces, and its IVs are
 * its tags.  An EAX decryption writes only authentic records, so its output starts as the caller's buffer. */
static int eax_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_eax_batch(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, b->decrypt, a[AB_NONCES].d, b->side[AB_NONCES].each, a[AB_AAD].d,
                           b->side[AB_AAD].each, b->nmsg, b->msg_bytes, t->d_in, t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d,
                           L->d_status);
}

static int siv_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_s2v_batch(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, &ks[1]->ek, b->decrypt, wipe_on_auth_failure(), a[AB_AAD].d,
                           b->side[AB_AAD].each, b->nmsg, b->msg_bytes, t->d_in, t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d,
                           L->d_status);
}

static int eax_siv_batch(int siv, int decrypt, int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                         const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                         const void *in, void *outp, uint8_t *tags, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = siv ? "siv batch" : "eax batch", .launch = siv ? siv_batch_launch : eax_batch_launch,
        .nkeys = siv ? 2 : 1, .keybits = keybits, .key = key, .decrypt = decrypt, .prefill = decrypt && !siv,
        .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_NONCES] = { nonces, nonce_len }, [AB_AAD] = { aData, aad_bytes }, [AB_TAGS] = { tags, 16 },
                  [AB_VERDICTS] = { verdicts, decrypt } } };
    return aead_rows_run(&b);
}

int uaes_eax_encrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                           const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags)
{
    return eax_siv_batch(0, 0, keybits, key, nmsg, msg_bytes, nonces, nonce_len, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_eax_decrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                           const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return eax_siv_batch(0, 1, keybits, key, nmsg, msg_bytes, nonces, nonce_len, aData, aad_bytes, crtxt, pntxt,
                         (uint8_t *)tags, verdicts);
}

int uaes_siv_encrypt_batch(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes,
                           const void *aData, size_t aad_bytes, const void *pntxt, uint8_t *ivs, void *crtxt)
{
    return eax_siv_batch(1, 0, keybits, keys, nmsg, msg_bytes, NULL, 0, aData, aad_bytes, pntxt, crtxt, ivs, NULL);
}

int uaes_siv_decrypt_batch(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes,
                           const void *aData, size_t aad_bytes, const uint8_t *ivs, const void *crtxt, void *pntxt,
                           uint8_t *verdicts)
{
    return eax_siv_batch(1, 1, keybits, keys, nmsg, msg_bytes, NULL, 0, aData, aad_bytes, crtxt, pntxt, (uint8_t *)ivs,
                         verdicts);
}

/* EAX' batches (k_eaxp_batch, uaes_eax_siv.hip): no associated data, 4-byte macs, and a length per nonce (nlens) as well
 * as per text (lens).  A decryption writes only authentic records, so its output starts as the caller's buffer.  What
 * this call checks comes first: the slot sizes, the lengths; then aead_rows_run's order.  An array of lengths in host
 * memory is read here and an entry above its slot refused; one in device memory is read by the kernel alone, which takes
 * such an entry as the slot. */
static int eaxp_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_eaxp_batch(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, b->decrypt, a[AB_NONCES].d, b->side[AB_NONCES].each,
                            a[AB_NLENS].d, b->nmsg, b->msg_bytes, a[AB_LENS].d, t->d_in, t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d,
                            L->d_status);
}

static int eaxp_lens_ok(const char *what, const uint32_t *lens, size_t nmsg, size_t slot)
{
    size_t m;
    if (!lens) return 0;
    if (is_device_ptr(lens))
        return ((uintptr_t)lens & 3u) ? fail(UAES_E_ARG, "a device array of lengths must be 4-byte aligned") : 0;
    for (m = 0; m < nmsg; ++m)
        if (lens[m] > slot) return fail(UAES_E_ARG, "%s length %zu is %u, above its slot of %zu bytes", what, m, lens[m], slot);
    return 0;
}

static int eaxp_batch(int decrypt, int keybits, const uint8_t *key, size_t nmsg, size_t nonce_bytes, const uint32_t *nlens,
                      const uint8_t *nonces, size_t msg_bytes, const uint32_t *lens, const void *in, void *outp,
                      uint8_t *macs, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = "eax' batch", .launch = eaxp_batch_launch, .nkeys = 1, .keybits = keybits, .key = key, .decrypt = decrypt,
        .prefill = decrypt, .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_NONCES] = { nonces, nonce_bytes }, [AB_NLENS] = { nlens, nlens ? sizeof *nlens : 0 },
                  [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { macs, 4 },
                  [AB_VERDICTS] = { verdicts, decrypt && verdicts } } };      /* (a caller may do without verdicts) */
    int rc;
    if (msg_bytes > UINT32_MAX || nonce_bytes > UINT32_MAX)
        return fail(UAES_E_ARG, "a batch slot holds at most %u bytes (got %zu of text, %zu of nonce)", UINT32_MAX, msg_bytes, nonce_bytes);
    if (nmsg > (size_t)-1 / 8 / (msg_bytes > nonce_bytes ? msg_bytes | 4 : nonce_bytes | 4))     /* (before lens is walked) */
        return fail(UAES_E_ARG, "batch size overflows");
    if (nmsg && (rc = eaxp_lens_ok("nonce", nlens, nmsg, nonce_bytes)) != 0) return rc;
    if (nmsg && (rc = eaxp_lens_ok("text", lens, nmsg, msg_bytes)) != 0) return rc;
    return aead_rows_run(&b);
}

int uaes_eaxp_encrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t nonce_bytes, const uint32_t *nlens,
                            const uint8_t *nonces, size_t msg_bytes, const uint32_t *lens,
                            const void *pntxt, void *crtxt, uint8_t *macs)
{
    return eaxp_batch(0, keybits, key, nmsg, nonce_bytes, nlens, nonces, msg_bytes, lens, pntxt, crtxt, macs, NULL);
}

int uaes_eaxp_decrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t nonce_bytes, const uint32_t *nlens,
                            const uint8_t *nonces, size_t msg_bytes, const uint32_t *lens,
                            const void *crtxt, const uint8_t *macs, void *pntxt, uint8_t *verdicts)
{
    return eaxp_batch(1, keybits, key, nmsg, nonce_bytes, nlens, nonces, msg_bytes, lens, crtxt, pntxt, (uint8_t *)macs, verdicts);
}

/* SIV batches with the component vector and a length per record (k_s2v_batch_v): every record's AAD slot, sum(adLens)
 * bytes, is cut into the same nad components.  What this call checks comes first: the components, the slot size, a
 * device array of lengths; then aead_rows_run's order. */
static int siv_batch_v_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_s2v_batch_v(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, &ks[1]->ek, b->decrypt, wipe_on_auth_failure(), a[AB_AAD].d,
                             (unsigned)b->nad, b->ad_lens, b->nmsg, b->msg_bytes, a[AB_LENS].d, t->d_in, t->d_out, a[AB_TAGS].d,
                             a[AB_VERDICTS].d, L->d_status);
}

static int siv_batch_v(int decrypt, int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                       size_t nad, const size_t *adLens, const void *aData, const void *in, void *outp, uint8_t *ivs,
                       uint8_t *verdicts)
{
    aead_rows b = {
        .name = "siv batch", .launch = siv_batch_v_launch, .nkeys = 2, .keybits = keybits, .key = keys, .decrypt = decrypt,
        .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp, .nad = nad, .ad_lens = adLens,
        .side = { [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { ivs, 16 }, [AB_VERDICTS] = { verdicts, decrypt } } };
    size_t total;
    int rc;
    if ((rc = siv_components(nad, adLens, UAES_SIV_BATCH_AD_MAX, &total)) != 0) return rc;
    if (msg_bytes > UINT32_MAX)
        return fail(UAES_E_ARG, "a batch record holds at most %u bytes (got %zu)", UINT32_MAX, msg_bytes);
    if (lens && ((uintptr_t)lens & 3u) && is_device_ptr(lens))
        return fail(UAES_E_ARG, "a device array of lengths must be 4-byte aligned");
    b.side[AB_AAD].p = aData;
    b.side[AB_AAD].each = total;
    return aead_rows_run(&b);
}

int uaes_siv_encrypt_batch_v(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                             size_t nad, const size_t *adLens, const void *aData,
                             const void *pntxt, uint8_t *ivs, void *crtxt)
{
    return siv_batch_v(0, keybits, keys, nmsg, msg_bytes, lens, nad, adLens, aData, pntxt, crtxt, ivs, NULL);
}

int uaes_siv_decrypt_batch_v(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                             size_t nad, const size_t *adLens, const void *aData,
                             const uint8_t *ivs, const void *crtxt, void *pntxt, uint8_t *verdicts)
{
    return siv_batch_v(1, keybits, keys, nmsg, msg_bytes, lens, nad, adLens, aData, crtxt, pntxt, (uint8_t *)ivs, verdicts);
}

/* CCM batches (k_ccm_batch, uaes_mac.hip): the nonce and tag lengths are arguments, the tags are packed, tagLen bytes
 * each, and `lens` may give every record a length of its own.  Like the reference's CCM a decryption writes the text
 * before it knows the tag, so the output need not start as the caller's buffer. */
static int ccm_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_ccm_batch(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, b->decrypt, wipe_on_auth_failure(), a[AB_NONCES].d,
                           b->side[AB_NONCES].each, b->side[AB_TAGS].each, a[AB_AAD].d, b->side[AB_AAD].each, b->nmsg,
                           b->msg_bytes, a[AB_LENS].d, t->d_in, t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d, L->d_status);
}

static int ccm_batch(int decrypt, int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen, size_t nmsg,
                     size_t msg_bytes, const uint32_t *lens, const uint8_t *nonces, const void *aData, size_t aad_bytes,
                     const void *in, void *outp, uint8_t *tags, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = "ccm batch", .launch = ccm_batch_launch, .nkeys = 1, .keybits = keybits, .key = key, .decrypt = decrypt,
        .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_NONCES] = { nonces, nonceLen }, [AB_AAD] = { aData, aad_bytes },
                  [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { tags, tagLen }, [AB_VERDICTS] = { verdicts, decrypt } } };
    int rc;
    if ((rc = ccm_lens_ok(nonceLen, tagLen)) != 0) return rc;
    if (msg_bytes > UAES_CCM_BATCH_MAX)
        return fail(UAES_E_ARG, "a CCM batch record holds at most %zu bytes (got %zu)", (size_t)UAES_CCM_BATCH_MAX, msg_bytes);
    if (aad_bytes > 0xFEFF) return fail(UAES_E_ARG, "a CCM batch record takes at most 65279 bytes of AAD (got %zu)", aad_bytes);
    return aead_rows_run(&b);
}

int uaes_ccm_encrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags)
{
    return ccm_batch(0, keybits, key, nonceLen, tagLen, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_ccm_decrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return ccm_batch(1, keybits, key, nonceLen, tagLen, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, crtxt, pntxt,
                     (uint8_t *)tags, verdicts);
}

/* GCM-SIV batches (k_gcmsiv_batch, uaes_gcmsiv_batch.hip): as ccm_batch with 12-byte nonces and 16-byte tags.  `key` is
 * the MASTER key: only its schedule is made here, every record derives and expands its own keys in the kernel.  Like
 * the reference's GCM-SIV a decryption writes the text before it knows the tag. */
static int gcmsiv_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_gcmsiv_batch(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, b->decrypt, wipe_on_auth_failure(), a[AB_NONCES].d, a[AB_AAD].d,
                              b->side[AB_AAD].each, b->nmsg, b->msg_bytes, a[AB_LENS].d, t->d_in, t->d_out, a[AB_TAGS].d,
                              a[AB_VERDICTS].d, L->d_status);
}

static int gcmsiv_batch(int decrypt, int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                        const uint8_t *nonces, const void *aData, size_t aad_bytes, const void *in, void *outp,
                        uint8_t *tags, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = "gcm-siv batch", .launch = gcmsiv_batch_launch, .nkeys = 1, .keybits = keybits, .key = key, .decrypt = decrypt,
        .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_NONCES] = { nonces, 12 }, [AB_AAD] = { aData, aad_bytes },
                  [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { tags, 16 }, [AB_VERDICTS] = { verdicts, decrypt } } };
    if (msg_bytes > UAES_GCMSIV_BATCH_MAX)
        return fail(UAES_E_ARG, "a GCM-SIV batch record holds at most %zu bytes (got %zu)", (size_t)UAES_GCMSIV_BATCH_MAX, msg_bytes);
    if (aad_bytes > UAES_GCMSIV_BATCH_MAX)
        return fail(UAES_E_ARG, "a GCM-SIV batch record takes at most %zu bytes of AAD (got %zu)", (size_t)UAES_GCMSIV_BATCH_MAX, aad_bytes);
    return aead_rows_run(&b);
}

int uaes_gcmsiv_encrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                              const uint8_t *nonces, const void *aData, size_t aad_bytes,
                              const void *pntxt, void *crtxt, uint8_t *tags)
{
    return gcmsiv_batch(0, keybits, key, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_gcmsiv_decrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                              const uint8_t *nonces, const void *aData, size_t aad_bytes,
                              const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return gcmsiv_batch(1, keybits, key, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, crtxt, pntxt, (uint8_t *)tags,
                        verdicts);
}

/* Multi-key GCM batches (k_gcm_multikey, uaes_gcm_multikey.hip): as gcmsiv_batch with packed tags of tagLen bytes and
 * `keys` as one more side array, nmsg * keybits / 8 bytes in host or device memory -- no key is expanded here, every
 * record's schedule is made in the kernel, so keybits is validated on its own.  (A host key array's way through the
 * scratch, and how that copy is cleared: aead_rows_staged.)  Decrypt keeps N7 per record: the kernel writes an
 * authentic record only, so the output's staging starts as the caller's buffer, and uaes_set_wipe_on_auth_failure does
 * not apply. */
static int gcm_multikey_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a,
                                     const row_text *t)
{
    (void)ks;
    return uaesk_gcm_multikey_batch(L->stream, &c->tb, b->keybits / 32 + 6, b->decrypt, b->side[AB_TAGS].each, a[AB_KEYS].d,
                                    a[AB_NONCES].d, a[AB_AAD].d, b->side[AB_AAD].each, b->nmsg, b->msg_bytes, a[AB_LENS].d, t->d_in,
                                    t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d, L->d_status);
}

static int gcm_multikey_batch(int decrypt, int keybits, const uint8_t *keys, size_t tagLen, size_t nmsg, size_t msg_bytes,
                              const uint32_t *lens, const uint8_t *nonces, const void *aData, size_t aad_bytes,
                              const void *in, void *outp, uint8_t *tags, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = "gcm multi-key batch", .launch = gcm_multikey_batch_launch, .nkeys = 0, .keybits = keybits, .decrypt = decrypt,
        .prefill = decrypt, .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_KEYS] = { keys, (size_t)keybits / 8 }, [AB_NONCES] = { nonces, 12 }, [AB_AAD] = { aData, aad_bytes },
                  [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { tags, tagLen }, [AB_VERDICTS] = { verdicts, decrypt } } };
    if (keybits != 128 && keybits != 192 && keybits != 256) return fail(UAES_E_ARG, "key bits must be 128, 192 or 256 (got %d)", keybits);
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "a GCM tag has 1 to 16 bytes (got %zu)", tagLen);
    if (msg_bytes > UAES_GCM_MULTIKEY_BATCH_MAX)
        return fail(UAES_E_ARG, "a multi-key GCM batch record holds at most %zu bytes (got %zu)", (size_t)UAES_GCM_MULTIKEY_BATCH_MAX, msg_bytes);
    if (aad_bytes > UAES_GCM_MULTIKEY_BATCH_MAX)
        return fail(UAES_E_ARG, "a multi-key GCM batch record takes at most %zu bytes of AAD (got %zu)", (size_t)UAES_GCM_MULTIKEY_BATCH_MAX, aad_bytes);
    return aead_rows_run(&b);
}

int uaes_gcm_multikey_encrypt_batch(int keybits, const uint8_t *keys, size_t tagLen, size_t nmsg, size_t msg_bytes,
                                    const uint32_t *lens, const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                    const void *pntxt, void *crtxt, uint8_t *tags)
{
    return gcm_multikey_batch(0, keybits, keys, tagLen, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_gcm_multikey_decrypt_batch(int keybits, const uint8_t *keys, size_t tagLen, size_t nmsg, size_t msg_bytes,
                                    const uint32_t *lens, const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                    const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return gcm_multikey_batch(1, keybits, keys, tagLen, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, crtxt, pntxt,
                              (uint8_t *)tags, verdicts);
}

/* XAES-256-GCM batches (C2SP; k_xaes_gcm_batch, uaes_xaes.hip): as gcmsiv_batch with 24-byte nonces -- `key` is the
 * MASTER key, always 256 bits: only its schedule and CMAC's subkey K1 under it are made here, every record derives and
 * expands the key of its nonce in the kernel -- and decrypting as gcm_multikey_batch: the kernel writes an authentic
 * record only, so the output's staging starts as the caller's buffer and uaes_set_wipe_on_auth_failure does not apply. */
static int xaes_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    uint8_t k1[16];
    uaesk_block kb;
    int k;
    xaes_k1(ks[0], k1);
    memcpy(kb.w, k1, sizeof k1);                  /* little-endian words of the byte stream, as a schedule's */
    k = uaesk_xaes_gcm_batch(L->stream, &c->tb, &ks[0]->ek, &kb, b->decrypt, a[AB_NONCES].d, a[AB_AAD].d, b->side[AB_AAD].each,
                             b->nmsg, b->msg_bytes, a[AB_LENS].d, t->d_in, t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d, L->d_status);
    burn(k1, sizeof k1);
    burn(&kb, sizeof kb);
    return k;
}

static int xaes_batch(int decrypt, const uint8_t *key, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                      const uint8_t *nonces, const void *aData, size_t aad_bytes, const void *in, void *outp,
                      uint8_t *tags, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = "xaes-256-gcm batch", .launch = xaes_batch_launch, .nkeys = 1, .keybits = 256, .key = key, .decrypt = decrypt,
        .prefill = decrypt, .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_NONCES] = { nonces, 24 }, [AB_AAD] = { aData, aad_bytes },
                  [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { tags, 16 },
                  [AB_VERDICTS] = { verdicts, decrypt && verdicts } } };      /* (a caller may do without verdicts) */
    if (msg_bytes > UAES_XAES_GCM_BATCH_MAX)
        return fail(UAES_E_ARG, "an XAES-256-GCM batch record holds at most %zu bytes (got %zu)", (size_t)UAES_XAES_GCM_BATCH_MAX, msg_bytes);
    if (aad_bytes > UAES_XAES_GCM_BATCH_MAX)
        return fail(UAES_E_ARG, "an XAES-256-GCM batch record takes at most %zu bytes of AAD (got %zu)", (size_t)UAES_XAES_GCM_BATCH_MAX, aad_bytes);
    return aead_rows_run(&b);
}

int uaes_xaes256gcm_encrypt_batch(const uint8_t key[32], size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                                  const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                  const void *pntxt, void *crtxt, uint8_t *tags)
{
    return xaes_batch(0, key, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_xaes256gcm_decrypt_batch(const uint8_t key[32], size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                                  const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                  const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return xaes_batch(1, key, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, crtxt, pntxt, (uint8_t *)tags, verdicts);
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
    KEYSCHED(ks);
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
        case 0: return host_result(uaesh_cbc_encrypt(&hk, iVec, 1, 0, x, len, y));
        case 1: return host_result(uaesh_cbc_decrypt(&hk, iVec, 1, x, len, y));
        case 2: uaesh_cfb(&hk, iVec, 1, x, len, y); return host_result(0);
        case 3: uaesh_cfb(&hk, iVec, 0, x, len, y); return host_result(0);
        case 4: uaesh_ofb(&hk, iVec, x, len, y); return host_result(0);
        case 8: return host_result(uaesh_cbc_decrypt(&hk, iVec, 0, x, len, y));
        default: return host_result(uaesh_cbc_encrypt(&hk, iVec, 0, mode - 5, x, len, y));
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
        if ((rc = launched("feedback-mode", k)) != 0) break;
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
    KEYSCHED(ks);
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
        if ((rc = launched("batch", k)) != 0) break;
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
/* batches of the plain cipher modes (sixteen GPU lanes per record)             */
/* ------------------------------------------------------------------------ */
/* CBC decrypt (with the CS3 swap and without), CBC encrypt without it, CFB, OFB and CTR over nmsg records in slots of
 * msg_bytes, one launch of k_cipher_batch (uaes_cipher_batch.hip), always on the GPU.  mode = enum
 * uaes_cipher_batch_mode; ivs = 16 bytes per record (CTR: its first counter block).  The conventions are the AEAD record
 * batches': every array host or device memory at any byte offset, host arrays through the lane's scratch and staging
 * buffers (row_stage / row_texts / row_finish), `lens` as in the CCM batch -- with it a host-memory output starts as a
 * copy of the caller's buffer, so that what the kernel leaves unwritten stays the caller's.  No verdicts, no status
 * word.  The order is the AEAD batches' too: the sizes, the key, nothing more for no records, the pointers, and only
 * then the device. */
static int cipher_rows(int mode, int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg, size_t msg_bytes,
                       const uint32_t *lens, const void *in, void *outp)
{
    const int cbc = mode == UAES_CB_CBC_DEC || mode == UAES_CB_CBC_DEC_BLOCKS || mode == UAES_CB_CBC_ENC_BLOCKS;
    const size_t total = nmsg * msg_bytes;
    context *c;
    lane *L;
    KEYSCHED(ks);
    int rc, k, bad;
    if (cbc && (msg_bytes < 16 || msg_bytes % 16))
        return fail(UAES_E_ARG, "batched CBC: every message must be a whole number of blocks (got %zu bytes)", msg_bytes);
    if (!cbc && msg_bytes > UINT32_MAX)
        return fail(UAES_E_ARG, "a batch record holds at most %u bytes (got %zu)", UINT32_MAX, msg_bytes);
    if (nmsg > (size_t)-1 / 2 / (msg_bytes > 16 ? msg_bytes : 16))     /* / 2: the IVs, the lengths and their padding */
        return fail(UAES_E_ARG, "batch size overflows");
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if (total == 0) return 0;                                     /* no records, or records of no bytes */
    if (!ivs || !in || !outp) return fail(UAES_E_ARG, "NULL pointer");
    if (cbc) lens = NULL;
    if ((rc = enter(&c, &L)) != 0) return rc;
    row_array a[2] = { { ivs, nmsg * 16, 0, NULL }, { lens, lens ? nmsg * sizeof *lens : 0, 0, NULL } };
    row_text t = { in, outp, total, total, lens != NULL, NULL, NULL };
    if (lens && is_device_ptr(lens) && ((uintptr_t)lens & 3u)) {
        rc = fail(UAES_E_ARG, "a device array of lengths must be 4-byte aligned");
        goto out;
    }
    if ((rc = row_stage(L, a, 2, 0)) != 0) goto out;
    if ((rc = row_texts(L, &t)) != 0) goto out;
    k = uaesk_cipher_batch(L->stream, &c->tb, ks.nr, &ks.ek, &ks.dk, mode, a[0].d, nmsg, msg_bytes, a[1].d, t.d_in, t.d_out);
    if ((rc = launched("cipher batch", k)) != 0) goto out;
    rc = row_finish(L, &t, a, 2, 0, &bad);
out:
    DONE(L, rc);
}

int uaes_cbc_decrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const void *crtxt, void *pntxt)
{
    return cipher_rows(UAES_CB_CBC_DEC, keybits, key, ivs, nmsg, msg_bytes, NULL, crtxt, pntxt);
}

int uaes_cbc_encrypt_blocks_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                                  size_t msg_bytes, const void *pntxt, void *crtxt)
{
    return cipher_rows(UAES_CB_CBC_ENC_BLOCKS, keybits, key, ivs, nmsg, msg_bytes, NULL, pntxt, crtxt);
}

int uaes_cbc_decrypt_blocks_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                                  size_t msg_bytes, const void *crtxt, void *pntxt)
{
    return cipher_rows(UAES_CB_CBC_DEC_BLOCKS, keybits, key, ivs, nmsg, msg_bytes, NULL, crtxt, pntxt);
}

int uaes_cfb_encrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *pntxt, void *crtxt)
{
    return cipher_rows(UAES_CB_CFB_ENC, keybits, key, ivs, nmsg, msg_bytes, lens, pntxt, crtxt);
}

int uaes_cfb_decrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *crtxt, void *pntxt)
{
    return cipher_rows(UAES_CB_CFB_DEC, keybits, key, ivs, nmsg, msg_bytes, lens, crtxt, pntxt);
}

int uaes_ofb_xcrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                          size_t msg_bytes, const uint32_t *lens, const void *in, void *out)
{
    return cipher_rows(UAES_CB_OFB, keybits, key, ivs, nmsg, msg_bytes, lens, in, out);
}

int uaes_ctr_xcrypt_batch(int keybits, const uint8_t *key, const uint8_t *ctrs, size_t nmsg,
                          size_t msg_bytes, const uint32_t *lens, const void *in, void *out)
{
    return cipher_rows(UAES_CB_CTR, keybits, key, ctrs, nmsg, msg_bytes, lens, in, out);
}

/* ------------------------------------------------------------------------ */
/* key wrap, RFC 3394 (AES_KEY_wrap / AES_KEY_unwrap, micro_aes.c:1829-1894),   */
/* and key wrap with padding, RFC 5649 / SP 800-38F KWP (the reference has none) */
/* ------------------------------------------------------------------------ */
/* One serial chain of 6 n block operations, one wave (uaes_kw.hip).  A secret of at most UAES_KW_LDS_MAX bytes in host
 * memory travels like any short text (plan_io: the mapped pinned buffers); the kernel reads all of it before it writes,
 * so plan_io's one staging buffer for both directions is fine.  A longer one is worked on in place in the output
 * buffer, which therefore is device memory of its own -- never the mapped host window, and never the input's staging
 * buffer (the secret sits 8 bytes into the wrapped form).  Device buffers go to the kernels as they are, at any byte
 * offset, the in-place form secret == wrapped + 8 included.  secret_len: padded. */
static int kw_io(lane *L, const void *in, size_t in_len, void *out, size_t out_len, size_t secret_len, io_plan *io)
{
    void *d_in, *d_out;
    int rc;
    if (secret_len <= UAES_KW_LDS_MAX && !(is_device_ptr(in) && is_device_ptr(out)))
        return plan_io(L, in, in_len, out, out_len, io);
    memset(io, 0, sizeof *io);
    if ((rc = stage_text(L, 0, in, in_len, 1, &d_in)) != 0) return rc;
    if ((rc = stage_text(L, 1, out, out_len, 0, &d_out)) != 0) return rc;
    io->din = d_in;
    io->dout = d_out;
    io->user_out = out;
    io->L = L;
    io->out_is_host = !is_device_ptr(out);
    io->copy_back = io->out_is_host;
    return 0;
}

/* What the two modes differ in once a call's arguments have passed its own checks.  Padding adds a secret of any length,
 * the one-block case and a verdict of three conditions, all in the kernel and the host path; here it shows as a second
 * status word, the length indicator, which the unwrap reports. */
typedef struct {
    int pad;                                       /* the kernels' switch; 1 + pad status words */
    const char *wrap, *unwrap, *batch;             /* what launched() calls the kernels */
    int (*host_wrap)(const uaesh_key *k, const uint8_t *secret, size_t len, uint8_t *wrapped);
    int (*host_unwrap)(const uaesh_key *k, const uint8_t *wrapped, size_t wrap_len, uint8_t *secret, uint32_t *secret_len);
} kw_mode;

static int kw_host_unwrap(const uaesh_key *k, const uint8_t *wrapped, size_t wrap_len, uint8_t *secret, uint32_t *secret_len)
{
    (void)secret_len;
    return uaesh_kw_unwrap(k, wrapped, wrap_len, secret);
}

static const kw_mode KW = { 0, "key wrap", "key unwrap", "key wrap batch", uaesh_kw_wrap, kw_host_unwrap };
static const kw_mode KWP = { 1, "key wrap with padding", "key unwrap with padding", "key wrap with padding batch",
                             uaesh_kwp_wrap, uaesh_kwp_unwrap };

/* out_len = bytes of the wrapped form; host_len = the length the host policy goes by */
static int kw_wrap(const kw_mode *m, const keysched *ks, const void *secret, size_t secretLen, void *wrapped, size_t out_len,
                   size_t host_len)
{
    context *c;
    lane *L;
    io_plan io;
    int rc;
    if (host_take(secret, wrapped, host_len, 1)) {
        const uaesh_key hk = host_key(ks);
        return host_result(m->host_wrap(&hk, (const uint8_t *)secret, secretLen, (uint8_t *)wrapped));
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = kw_io(L, secret, secretLen, wrapped, out_len, out_len - 8, &io)) != 0) break;
        int k = uaesk_kw(L->stream, &c->tb, ks->nr, &ks->ek, &ks->dk, m->pad, 0, io.din, secretLen, io.dout, NULL);
        if ((rc = launched(m->wrap, k)) != 0) break;
        rc = finish_io(&io, out_len);
    } while (0);
    DONE(L, rc);
}

/* secretLen (padding; else NULL) receives the length indicator of an authentic secret */
static int kw_unwrap(const kw_mode *m, const keysched *ks, const void *wrapped, size_t wrapLen, void *secret, size_t *secretLen)
{
    context *c;
    lane *L;
    io_plan io;
    int rc, status[2] = { 0, 0 };
    const size_t len = wrapLen - 8;
    if (host_take(wrapped, secret, wrapLen, 1)) {
        const uaesh_key hk = host_key(ks);
        uint32_t mli = 0;
        rc = m->host_unwrap(&hk, (const uint8_t *)wrapped, wrapLen, (uint8_t *)secret, &mli);
        if (rc == UAES_E_AUTHENTICATION && wipe_on_auth_failure()) memset(secret, 0, len);   /* (the default leaves it, as the reference does) */
        if (secretLen) *secretLen = mli;
        return host_result(rc);
    }
    if ((rc = enter(&c, &L)) != 0) return rc;
    do {
        if ((rc = kw_io(L, wrapped, wrapLen, secret, len, len, &io)) != 0) break;
        int k = uaesk_kw(L->stream, &c->tb, ks->nr, &ks->ek, &ks->dk, m->pad, 1, io.din, len, io.dout, L->d_status);
        if ((rc = launched(m->unwrap, k)) != 0) break;
        if ((rc = lane_fetch(L, status, L->d_status, (1 + m->pad) * sizeof status[0])) != 0) break;
        io.drained = 1;
        /* like the reference: the secret is written before A is checked; SABOTAGE = uaes_set_wipe_on_auth_failure */
        if ((rc = status[0] ? finish_io_unauthenticated(&io, len) : finish_io(&io, len)) != 0) break;
        if (status[0]) rc = UAES_E_AUTHENTICATION;
        else if (secretLen) *secretLen = (uint32_t)status[1];
    } while (0);
    DONE(L, rc);
}

int uaes_kw_wrap(int keybits, const uint8_t *kek, const void *secret, size_t secretLen, void *wrapped)
{
    KEYSCHED(ks);
    int rc;
    if ((rc = expand_key(&ks, kek, keybits)) != 0) return rc;
    if (secretLen % 8 || secretLen / 8 < 2) return UAES_E_DATALENGTH;     /* (:1837) */
    if (!secret || !wrapped) return fail(UAES_E_ARG, "NULL pointer");
    if (secretLen > (size_t)-1 - 8) return fail(UAES_E_ARG, "length overflows");
    return kw_wrap(&KW, &ks, secret, secretLen, wrapped, secretLen + 8, secretLen);
}

int uaes_kw_unwrap(int keybits, const uint8_t *kek, const void *wrapped, size_t wrapLen, void *secret)
{
    KEYSCHED(ks);
    int rc;
    if ((rc = expand_key(&ks, kek, keybits)) != 0) return rc;
    if (wrapLen % 8 || wrapLen / 8 < 3) return UAES_E_DATALENGTH;        /* (:1873) */
    if (!secret || !wrapped) return fail(UAES_E_ARG, "NULL pointer");
    return kw_unwrap(&KW, &ks, wrapped, wrapLen, secret, NULL);
}

int uaes_kwp_wrap(int keybits, const uint8_t *kek, const void *secret, size_t secretLen, void *wrapped)
{
    KEYSCHED(ks);
    int rc;
    const size_t out_len = uaes_kwp_wrapped_len(secretLen);
    if ((rc = expand_key(&ks, kek, keybits)) != 0) return rc;
    if (out_len == 0) return UAES_E_DATALENGTH;
    if (!secret || !wrapped) return fail(UAES_E_ARG, "NULL pointer");
    return kw_wrap(&KWP, &ks, secret, secretLen, wrapped, out_len, out_len);
}

int uaes_kwp_unwrap(int keybits, const uint8_t *kek, const void *wrapped, size_t wrapLen, void *secret, size_t *secretLen)
{
    KEYSCHED(ks);
    int rc;
    if ((rc = expand_key(&ks, kek, keybits)) != 0) return rc;
    if (wrapLen % 8 || wrapLen < 16 || (uint64_t)(wrapLen - 8) > (uint64_t)1 << 32) return UAES_E_DATALENGTH;
    if (!secret || !wrapped || !secretLen) return fail(UAES_E_ARG, "NULL pointer");
    *secretLen = 0;
    return kw_unwrap(&KWP, &ks, wrapped, wrapLen, secret, secretLen);
}

/* Batches: nkeys slots under one key-encryption key, sixteen lanes per record, always on the GPU.  rec = bytes of a
 * secret's slot (unwrap: the wrapped slot - 8).  Padding gives each record a length of its own (lens, NULL: every record
 * fills its slot) and reports the secrets' lengths (lens_out); without it both are NULL.  Any array may be host or device
 * memory; host arrays travel through the lane's staging buffers.  The status word takes two bits: 1 for a record that
 * does not authenticate, 2 for a wrap length of 0 or beyond the slot. */
static int kw_batch(const kw_mode *m, int unwrap, int keybits, const uint8_t *kek, size_t nkeys, size_t rec, const uint32_t *lens,
                    const void *in, void *outp, uint32_t *lens_out, uint8_t *verdicts)
{
    context *c;
    lane *L;
    KEYSCHED(ks);
    int rc, k, bad;
    const size_t wslot = (rec + 7) / 8 * 8 + 8, in_rec = unwrap ? wslot : rec, out_rec = unwrap ? rec : wslot;
    const int status = unwrap || lens != NULL;
    if ((rc = expand_key(&ks, kek, keybits)) != 0) return rc;
    if (rec > UAES_KW_BATCH_MAX)                          /* (key wrap with padding has refused it before the key) */
        return fail(UAES_E_ARG, "batched key wrap: a record holds at most %zu bytes of secret (got %zu)",
                    (size_t)UAES_KW_BATCH_MAX, rec);
    if (nkeys > (size_t)-1 / wslot) return fail(UAES_E_ARG, "batch size overflows");
    if (nkeys == 0) return 0;
    if (!in || !outp || (unwrap && (!verdicts || (m->pad && !lens_out)))) return fail(UAES_E_ARG, "NULL pointer");
    if ((rc = enter(&c, &L)) != 0) return rc;
    row_array a[3] = { { lens, lens ? nkeys * sizeof *lens : 0, 0, NULL }, { lens_out, lens_out ? nkeys * sizeof *lens_out : 0, 1, NULL },
                       { verdicts, unwrap ? nkeys : 0, 1, NULL } };
    /* with lens a record may leave part of its slot, or all of it, unwritten: a host output starts as the caller's bytes */
    row_text t = { in, outp, nkeys * in_rec, nkeys * out_rec, lens != NULL, NULL, NULL };
    if ((lens && is_device_ptr(lens) && ((uintptr_t)lens & 3u)) || (lens_out && is_device_ptr(lens_out) && ((uintptr_t)lens_out & 3u))) {
        rc = fail(UAES_E_ARG, "a device array of lengths must be 4-byte aligned");
        goto out;
    }
    /* a wrap without lens has nothing to report: no status word */
    if ((rc = row_stage(L, a, 3, status)) != 0) goto out;
    if ((rc = row_texts(L, &t)) != 0) goto out;
    k = uaesk_kw_batch(L->stream, &c->tb, ks.nr, &ks.ek, &ks.dk, m->pad, unwrap, wipe_on_auth_failure(), nkeys, rec, a[0].d,
                       t.d_in, t.d_out, a[1].d, a[2].d, L->d_status);
    if ((rc = launched(m->batch, k)) != 0) goto out;
    if ((rc = row_finish(L, &t, a, 3, status, &bad)) != 0) goto out;
    rc = (bad & 1) ? UAES_E_AUTHENTICATION : (bad & 2) ? UAES_E_DATALENGTH : 0;
out:
    DONE(L, rc);
}

int uaes_kw_wrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t secret_bytes, const void *secrets, void *wrapped)
{
    if (secret_bytes % 8 || secret_bytes / 8 < 2) return UAES_E_DATALENGTH;
    return kw_batch(&KW, 0, keybits, kek, nkeys, secret_bytes, NULL, secrets, wrapped, NULL, NULL);
}

int uaes_kw_unwrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t wrapped_bytes, const void *wrapped,
                         void *secrets, uint8_t *verdicts)
{
    if (wrapped_bytes % 8 || wrapped_bytes / 8 < 3) return UAES_E_DATALENGTH;
    return kw_batch(&KW, 1, keybits, kek, nkeys, wrapped_bytes - 8, NULL, wrapped, secrets, NULL, verdicts);
}

int uaes_kwp_wrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t secret_bytes, const uint32_t *lens,
                        const void *secrets, void *wrapped)
{
    if (secret_bytes == 0 || secret_bytes > UAES_KW_BATCH_MAX)
        return fail(UAES_E_ARG, "batched key wrap with padding: a record holds 1 .. %zu bytes of secret (got %zu)",
                    (size_t)UAES_KW_BATCH_MAX, secret_bytes);
    return kw_batch(&KWP, 0, keybits, kek, nkeys, secret_bytes, lens, secrets, wrapped, NULL, NULL);
}

int uaes_kwp_unwrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t wrapped_bytes, const uint32_t *wlens,
                          const void *wrapped, void *secrets, uint32_t *lens_out, uint8_t *verdicts)
{
    if (wrapped_bytes % 8 || wrapped_bytes < 16 || wrapped_bytes > UAES_KW_BATCH_MAX + 8)
        return fail(UAES_E_ARG, "batched key unwrap with padding: a wrapped record is a multiple of 8 in 16 .. %zu bytes (got %zu)",
                    (size_t)UAES_KW_BATCH_MAX + 8, wrapped_bytes);
    return kw_batch(&KWP, 1, keybits, kek, nkeys, wrapped_bytes - 8, wlens, wrapped, secrets, lens_out, verdicts);
}

/* ------------------------------------------------------------------------ */
/* FF1, SP 800-38G (AES_FPE_encrypt / AES_FPE_decrypt, micro_aes.c:2091-2147, :2267-2347) */
/* ------------------------------------------------------------------------ */
/* Kernels in uaes_ff1.hip.  What depends on (radix, alphabet, len, tweak length) alone is made here, once per call: the
 * two alphabet tables, b and d with exact integers (uaesh_ff1_b -- not the reference's floating-point LOGRDX form,
 * DESIGN.md), the P block.  cap = the longest text this call takes. */
/* the two tables as the host path makes them (uaesh_fpe_alphabet), with the engine's messages */
static int fpe_alphabet(const char *mode, unsigned radix, const uint8_t *alphabet, uint8_t inv[256], uint8_t fwd[256])
{
    int twice;
    if (radix < 2 || radix > 256) return fail(UAES_E_ARG, "%s: radix %u (2..256)", mode, radix);
    if ((twice = uaesh_fpe_alphabet(radix, alphabet, inv, fwd)) >= 0)
        return fail(UAES_E_ARG, "%s: byte 0x%02x occurs twice in the alphabet", mode, twice);
    return 0;
}

static int ff1_setup(unsigned radix, const uint8_t *alphabet, size_t tweakLen, size_t tweak_stride, size_t len, size_t cap,
                     uaesk_ff1 *q)
{
    uint8_t p[16];
    size_t v;
    unsigned i;
    int rc;
    memset(q, 0, sizeof *q);
    if ((rc = fpe_alphabet("FF1", radix, alphabet, q->inv, q->fwd)) != 0) return rc;
    if (len < uaesh_ff1_minlen(radix) || len > cap || (uint64_t)tweakLen >> 32) return UAES_E_DATALENGTH;
    v = len - len / 2;
    q->radix = radix;
    q->len = (unsigned)len;
    q->b = (unsigned)uaesh_ff1_b(radix, v);
    q->d = 4 * ((q->b + 3) / 4) + 4;
    q->tweak_len = tweakLen;
    q->tweak_stride = tweak_stride;
    p[0] = 1; p[1] = 2; p[2] = 1; p[3] = (uint8_t)(radix >> 16); p[4] = (uint8_t)(radix >> 8); p[5] = (uint8_t)radix;
    p[6] = 10; p[7] = (uint8_t)(len / 2);
    for (i = 0; i < 4; ++i) { p[8 + i] = (uint8_t)(len >> (24 - 8 * i)); p[12 + i] = (uint8_t)(tweakLen >> (24 - 8 * i)); }
    for (i = 0; i < 4; ++i) q->p[i] = (unsigned)p[4 * i] | (unsigned)p[4 * i + 1] << 8 | (unsigned)p[4 * i + 2] << 16 | (unsigned)p[4 * i + 3] << 24;
    return 0;
}

/* FF1 (f1) or FF3-1 (f3, f1 NULL).  nrec 0: one text.  Host arrays travel through the lane's staging buffers; the
 * output's buffer starts as a copy of the caller's, so that a record the kernel leaves unwritten comes back as it was. */
static int fpe_gpu(const keysched *ks, int decrypt, const uaesk_ff1 *f1, const uaesk_ff3 *f3, const uint8_t *tweaks,
                   size_t tweak_bytes, size_t nrec, const void *in, void *outp, uint8_t *verdicts)
{
    context *c;
    lane *L;
    const void *d_tweaks = NULL;
    const size_t n = nrec ? nrec : 1, total = n * (f1 ? f1->len : f3->len);
    int rc, k, bad;
    if ((rc = enter(&c, &L)) != 0) return rc;
    row_array a[1] = { { verdicts, verdicts ? n : 0, 1, NULL } };
    row_text t = { in, outp, total, total, 1, NULL, NULL };
    if ((rc = row_stage(L, a, 1, 1)) != 0) goto out;
    if ((rc = stage_aad(L, tweaks, tweak_bytes, &d_tweaks)) != 0) goto out;
    if ((rc = row_texts(L, &t)) != 0) goto out;
    if (f1) k = uaesk_ff1_run(L->stream, &c->tb, ks->nr, &ks->ek, decrypt, f1, d_tweaks, nrec, t.d_in, t.d_out, a[0].d, L->d_status);
    else k = uaesk_ff3_run(L->stream, &c->tb, ks->nr, &ks->ek, decrypt, f3, d_tweaks, nrec, t.d_in, t.d_out, a[0].d, L->d_status);
    if ((rc = launched(f1 ? "FF1" : "FF3-1", k)) != 0) goto out;
    if ((rc = row_finish(L, &t, a, 1, 1, &bad)) != 0) goto out;
    rc = bad ? (decrypt ? UAES_E_DECRYPTION : UAES_E_ENCRYPTION) : 0;
out:
    DONE(L, rc);
}

/* what a batch checks once its setup has passed and nrec is not 0; tweakLen 0: no tweaks.  *tweak_bytes = their span */
static int fpe_batch_args(size_t nrec, size_t len, size_t tweakLen, size_t tweak_stride, const void *tweaks,
                          const void *in, const void *out, size_t *tweak_bytes)
{
    if (nrec > (size_t)-1 / len || (tweak_stride && nrec - 1 > ((size_t)-1 - tweakLen) / tweak_stride))
        return fail(UAES_E_ARG, "batch size overflows");
    if (!in || !out || (tweakLen && !tweaks)) return fail(UAES_E_ARG, "NULL pointer");
    *tweak_bytes = tweakLen ? (nrec - 1) * tweak_stride + tweakLen : 0;
    return 0;
}

/* the host path's answer: a byte that is no numeral is the caller's code, anything else goes through host_result */
static int fpe_host_result(int rc)
{
    return rc == UAES_E_ENCRYPTION || rc == UAES_E_DECRYPTION ? rc : host_result(rc);
}

static int ff1_one(int decrypt, int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                   const uint8_t *tweak, size_t tweakLen, const void *in, size_t len, void *out)
{
    KEYSCHED(ks);
    uaesk_ff1 q;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if ((rc = ff1_setup(radix, alphabet, tweakLen, 0, len, UAES_FF1_MAX, &q)) != 0) return rc;
    if (!in || !out || (tweakLen && !tweak)) return fail(UAES_E_ARG, "NULL pointer");
    if (host_take(in, out, len, 1) && !(tweakLen && is_device_ptr(tweak))) {
        const uaesh_key hk = host_key(&ks);
        return fpe_host_result(uaesh_ff1(&hk, decrypt, radix, alphabet, tweak, tweakLen, (const uint8_t *)in, len, (uint8_t *)out));
    }
    return fpe_gpu(&ks, decrypt, &q, NULL, tweak, tweakLen, 0, in, out, NULL);
}

int uaes_ff1_encrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak, size_t tweakLen, const void *in, size_t len, void *out)
{
    return ff1_one(0, keybits, key, radix, alphabet, tweak, tweakLen, in, len, out);
}

int uaes_ff1_decrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak, size_t tweakLen, const void *in, size_t len, void *out)
{
    return ff1_one(1, keybits, key, radix, alphabet, tweak, tweakLen, in, len, out);
}

static int ff1_batch(int decrypt, int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweaks, size_t tweakLen, size_t tweak_stride, size_t nrec, size_t len,
                     const void *in, void *out, uint8_t *verdicts)
{
    KEYSCHED(ks);
    uaesk_ff1 q;
    size_t tweak_bytes;
    int rc;
    if ((rc = expand_key(&ks, key, keybits)) != 0) return rc;
    if ((rc = ff1_setup(radix, alphabet, tweakLen, tweak_stride, len, UAES_FF1_BATCH_MAX, &q)) != 0) return rc;
    if (nrec == 0) return 0;
    if ((rc = fpe_batch_args(nrec, len, tweakLen, tweak_stride, tweaks, in, out, &tweak_bytes)) != 0) return rc;
    return fpe_gpu(&ks, decrypt, &q, NULL, tweaks, tweak_bytes, nrec, in, out, verdicts);
}

int uaes_ff1_encrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweakLen, size_t tweak_stride,
                           size_t nrec, size_t len, const void *in, void *out, uint8_t *verdicts)
{
    return ff1_batch(0, keybits, key, radix, alphabet, tweaks, tweakLen, tweak_stride, nrec, len, in, out, verdicts);
}

int uaes_ff1_decrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweakLen, size_t tweak_stride,
                           size_t nrec, size_t len, const void *in, void *out, uint8_t *verdicts)
{
    return ff1_batch(1, keybits, key, radix, alphabet, tweaks, tweakLen, tweak_stride, nrec, len, in, out, verdicts);
}

/* ------------------------------------------------------------------------ */
/* FF3-1, SP 800-38G revision 1 (AES_FPE_encrypt / AES_FPE_decrypt with FF_X 3, micro_aes.c:2150-2248, :2267-2347) */
/* ------------------------------------------------------------------------ */
/* Kernel in uaes_ff3.hip.  The cipher runs under the key with its bytes reversed: ks = that key's schedule, for the GPU
 * and for the host path alike. */
static int ff3_setup(keysched *ks, int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     size_t tweak_stride, size_t len, uaesk_ff3 *q)
{
    uint8_t rev[32];
    unsigned i;
    int rc;
    if ((keybits != 128 && keybits != 192 && keybits != 256) || !key) return expand_key(ks, key, keybits);   /* its error */
    for (i = 0; i < (unsigned)keybits / 8; ++i) rev[i] = key[keybits / 8 - 1 - i];
    rc = expand_key(ks, rev, keybits);
    burn(rev, sizeof rev);
    if (rc) return rc;
    memset(q, 0, sizeof *q);
    if ((rc = fpe_alphabet("FF3-1", radix, alphabet, q->inv, q->fwd)) != 0) return rc;
    if (len < uaesh_ff1_minlen(radix) || len > uaesh_ff3_maxlen(radix)) return UAES_E_DATALENGTH;
    q->radix = radix;
    q->len = (unsigned)len;
    q->tweak_stride = tweak_stride;
    return 0;
}

static int ff3_one(int decrypt, int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                   const uint8_t *tweak, const void *in, size_t len, void *out)
{
    KEYSCHED(ks);
    uaesk_ff3 q;
    int rc;
    if ((rc = ff3_setup(&ks, keybits, key, radix, alphabet, 0, len, &q)) != 0) return rc;
    if (!in || !out || !tweak) return fail(UAES_E_ARG, "NULL pointer");
    if (host_take(in, out, len, 1) && !is_device_ptr(tweak)) {
        const uaesh_key hk = host_key(&ks);
        return fpe_host_result(uaesh_ff3(&hk, decrypt, radix, alphabet, tweak, (const uint8_t *)in, len, (uint8_t *)out));
    }
    return fpe_gpu(&ks, decrypt, NULL, &q, tweak, UAES_FF3_TWEAK, 0, in, out, NULL);
}

size_t uaes_ff3_maxlen(unsigned radix) { return uaesh_ff3_maxlen(radix); }

int uaes_ff3_encrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak, const void *in, size_t len, void *out)
{
    return ff3_one(0, keybits, key, radix, alphabet, tweak, in, len, out);
}

int uaes_ff3_decrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak, const void *in, size_t len, void *out)
{
    return ff3_one(1, keybits, key, radix, alphabet, tweak, in, len, out);
}

static int ff3_batch(int decrypt, int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweaks, size_t tweak_stride, size_t nrec, size_t len,
                     const void *in, void *out, uint8_t *verdicts)
{
    KEYSCHED(ks);
    uaesk_ff3 q;
    size_t tweak_bytes;
    int rc;
    if ((rc = ff3_setup(&ks, keybits, key, radix, alphabet, tweak_stride, len, &q)) != 0) return rc;
    if (nrec == 0) return 0;
    if ((rc = fpe_batch_args(nrec, len, UAES_FF3_TWEAK, tweak_stride, tweaks, in, out, &tweak_bytes)) != 0) return rc;
    return fpe_gpu(&ks, decrypt, NULL, &q, tweaks, tweak_bytes, nrec, in, out, verdicts);
}

int uaes_ff3_encrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweak_stride, size_t nrec, size_t len,
                           const void *in, void *out, uint8_t *verdicts)
{
    return ff3_batch(0, keybits, key, radix, alphabet, tweaks, tweak_stride, nrec, len, in, out, verdicts);
}

int uaes_ff3_decrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweak_stride, size_t nrec, size_t len,
                           const void *in, void *out, uint8_t *verdicts)
{
    return ff3_batch(1, keybits, key, radix, alphabet, tweaks, tweak_stride, nrec, len, in, out, verdicts);
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
    KEYSCHED(ks);
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
        return host_result(rc);
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
        if ((rc = launched("ocb", k)) != 0) break;
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

/* OCB batches (k_ocb_batch, uaes_ocb.hip): as ccm_batch (aead_rows_run), with OCB's nonce and tag lengths and both key
 * schedules (a decrypting record needs the inverse cipher for its text and the forward one for K_top, HASH, the pad and
 * the tag).  Like the reference's OCB a decryption writes the text before it knows the tag.  The batch always runs on
 * the GPU: the host policy of the one-message calls does not apply. */
static int ocb_batch_launch(const aead_rows *b, context *c, lane *L, const keysched *const ks[2], const row_array *a, const row_text *t)
{
    return uaesk_ocb_batch(L->stream, &c->tb, ks[0]->nr, &ks[0]->ek, &ks[0]->dk, b->decrypt, wipe_on_auth_failure(), a[AB_NONCES].d,
                           b->side[AB_NONCES].each, b->side[AB_TAGS].each, a[AB_AAD].d, b->side[AB_AAD].each, b->nmsg,
                           b->msg_bytes, a[AB_LENS].d, t->d_in, t->d_out, a[AB_TAGS].d, a[AB_VERDICTS].d, L->d_status);
}

static int ocb_batch(int decrypt, int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen, size_t nmsg,
                     size_t msg_bytes, const uint32_t *lens, const uint8_t *nonces, const void *aData, size_t aad_bytes,
                     const void *in, void *outp, uint8_t *tags, uint8_t *verdicts)
{
    const aead_rows b = {
        .name = "ocb batch", .launch = ocb_batch_launch, .nkeys = 1, .keybits = keybits, .key = key, .decrypt = decrypt,
        .nmsg = nmsg, .msg_bytes = msg_bytes, .in = in, .out = outp,
        .side = { [AB_NONCES] = { nonces, nonceLen }, [AB_AAD] = { aData, aad_bytes },
                  [AB_LENS] = { lens, lens ? sizeof *lens : 0 }, [AB_TAGS] = { tags, tagLen }, [AB_VERDICTS] = { verdicts, decrypt } } };
    if (nonceLen < 1 || nonceLen > 15) return fail(UAES_E_ARG, "OCB nonce length %zu (1..15)", nonceLen);
    if (tagLen < 1 || tagLen > 16) return fail(UAES_E_ARG, "OCB tag length %zu (1..16)", tagLen);
    if (msg_bytes > UAES_OCB_BATCH_MAX)
        return fail(UAES_E_ARG, "an OCB batch record holds at most %zu bytes (got %zu)", (size_t)UAES_OCB_BATCH_MAX, msg_bytes);
    if (aad_bytes > UAES_OCB_BATCH_MAX)
        return fail(UAES_E_ARG, "an OCB batch record takes at most %zu bytes of AAD (got %zu)", (size_t)UAES_OCB_BATCH_MAX, aad_bytes);
    return aead_rows_run(&b);
}

int uaes_ocb_encrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags)
{
    return ocb_batch(0, keybits, key, nonceLen, tagLen, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, pntxt, crtxt, tags, NULL);
}

int uaes_ocb_decrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts)
{
    return ocb_batch(1, keybits, key, nonceLen, tagLen, nmsg, msg_bytes, lens, nonces, aData, aad_bytes, crtxt, pntxt,
                     (uint8_t *)tags, verdicts);
}

int uaes_ocb_dev(int keybits, const uint8_t *key, const uint8_t *nonce, int decrypt,
                 const void *d_aad, size_t aad_len,
                 const void *d_in, size_t len, void *d_out, int *d_status, void *stream)
{
    context *c;
    KEYSCHED(ks);
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
