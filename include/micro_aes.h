/*
 * micro_aes.h -- drop-in replacement for the reference's public header, for
 * the modes served by the MI355X engine (ECB, CTR, XTS, GCM on the
 * block-parallel hot path; CMAC and CCM for the remaining NIST .rsp files;
 * CBC, CFB, OFB with their parallel decrypt directions).
 *
 * Same function names, argument order, return types and configuration macros
 * as polfosol/micro-AES v11 (micro_aes.h:17-129, :173-181, :239-249, :256-266,
 * :294-308, :469-476), so that callers written against the reference -- its
 * main.c and its testvectors/ harness -- compile unchanged and link against
 * libmicro_aes_hip_<bits>.so instead of micro_aes.c.  Modes the engine does
 * not implement have their macro set to 0, which is how the reference itself
 * switches a mode (and the harness's test for it) off.
 *
 * The AES_* functions below are thin wrappers (uaes_compat.c) around the
 * run-time-key-size C ABI in uaes_hip.h; buffers may be host or HIP device
 * memory.  On an engine failure (no GPU, HIP error) the void functions print a
 * diagnostic and abort() -- they never return unencrypted data -- and the
 * char functions return M_ENCRYPTION_ERROR / M_DECRYPTION_ERROR.
 */
#ifndef MICRO_AES_H_
#define MICRO_AES_H_

#ifndef AES___
#define AES___ 128 /* or 192 / 256 (also settable with -DAES___=...); must match the library linked */
#endif

#define BLOCKCIPHERS 1
#define AEAD_MODES   1

#define ECB      1
#define CTR      1
#define CTR_NA   1
#define XEX      1
#define XTS      1
#define GCM      1
#define CMAC     1          /* serial CBC-MAC chains: one GPU lane (uaes_mac.hip) */
#define CCM      1
#define GCM_SIV  1          /* RFC 8452: POLYVAL through the GHASH kernels, LE32 counter */

#define CBC      1          /* feedback modes: decrypt of CBC/CFB is block-   */
#define CFB      1          /* parallel, the rest one GPU lane (uaes_chain.hip) */
#define OFB      1
#ifndef CTS                  /* micro_aes.h:56 -- CBC ciphertext stealing (CS3).  A caller built with -DCTS=0 gets   */
#define CTS      1          /* the reference's other CBC: last chunk padded (AES_PADDING), whole-block decrypt   */
#endif
#ifndef KWA                  /* micro_aes.h:50 -- key wrap, RFC 3394 (uaes_kw.hip); every library exports AES_KEY_wrap /  */
#define KWA      0          /* AES_KEY_unwrap, a caller built with -DKWA=1 sees the prototypes (below)                */
#endif
#ifndef FPE                  /* micro_aes.h:51 -- FF1 / FF3-1 format-preserving encryption (uaes_ff1.hip, uaes_ff3.hip); every library exports */
#define FPE      0          /* AES_FPE_* and AES_FF3_*, a caller built with -DFPE=1 sees the prototypes (below)    */
#endif
#if FPE
#ifndef CUSTOM_ALPHABET      /* micro_aes.h:87 -- 0: the digits 0..9; 1..9: ALPHABET and RADIX of the caller's micro_fpe.h */
#define CUSTOM_ALPHABET 0
#endif
#ifndef FF_X                 /* micro_aes.h:88 -- 1: FF1, the only method AES_FPE_* is bound to (FF3-1: AES_FF3_*) */
#define FF_X            1
#endif
#if FF_X != 1
#error "FF_X: AES_FPE_* is bound to FF1 (FF_X 1) only; FF3-1 is served through AES_FF3_encrypt / AES_FF3_decrypt"
#endif
#if CUSTOM_ALPHABET >= 10 || CUSTOM_ALPHABET < 0
#error "CUSTOM_ALPHABET: wide-character alphabets (10 and above) are not served"
#endif
#endif
#ifndef EAX                  /* micro_aes.h:43 -- EAX (uaes_eax_siv.hip); every library exports AES_EAX_*, a caller */
#define EAX      0          /* built with -DEAX=1 sees the prototypes (below)                                       */
#endif
#ifndef EAXP                 /* micro_aes.h:70 -- EAX', IEEE 1703 (uaes_eax_siv.hip); every library exports AES_EAXP_*, a */
#define EAXP     0          /* caller built with -DEAX=1 -DEAXP=1 gets AES_EAX_* with the EAX' parameter lists (below)  */
#endif
#ifndef SIV                  /* micro_aes.h:44 -- SIV, RFC 5297 (uaes_eax_siv.hip); every library exports AES_SIV_*, */
#define SIV      0          /* a caller built with -DSIV=1 sees the prototypes (below)                              */
#endif
#define OCB      1          /* RFC 7253: block-parallel, offsets from the Gray code (uaes_ocb.hip) */
#ifndef POLY1305             /* micro_aes.h:52 -- Poly1305-AES (uaes_poly1305.hip); every library exports        */
#define POLY1305 0          /* AES_Poly1305, a caller built with -DPOLY1305=1 sees its prototype (below)        */
#endif
#define MICRO_RJNDL 0

#ifndef AES_PADDING          /* micro_aes.h:79 -- 0 zeros, 1 PKCS#7, 2 ISO/IEC 7816-4; a caller */
#define AES_PADDING     0   /* built with -DAES_PADDING=1|2 gets that ECB padding (see below)   */
#endif
#define DECRYPTION      1
#ifndef PRESET_COUNTER       /* micro_aes.h:100 -- a caller built with -DPRESET_COUNTER=1 hands AES_CTR_* the    */
#define PRESET_COUNTER  0   /* whole 16-byte counter block instead of a 12-byte IV (micro_aes.c:965-966)     */
#endif

/* The reference fixes these lengths as enum constants that a user edits in its header (micro_aes.h:103-116).  Here a
 * caller built with -DCCM_NONCE_LEN=n (7..13), -DCCM_TAG_LEN=n (even, 4..16), -DGCM_NONCE_LEN=n (>= 1),
 * -DGCM_TAG_LEN=n (1..16), -DOCB_NONCE_LEN=n (1..15) or -DOCB_TAG_LEN=n (1..16) gets that build: the macro stands in
 * for the enum constant and the AES_CCM_* / AES_GCM_* / AES_OCB_* names bind to the general entry points below.    */
enum constant_parameters_of_modes
{
#ifndef CTR_START_VALUE    /* micro_aes.h:98-99; -DCTR_START_VALUE=n / -DCTR_IV_LENGTH=n (<= 16) bind AES_CTR_* to  */
    CTR_START_VALUE = 1,   /* the general entry point below (micro_aes.c:968-971)                                */
#endif
#ifndef CTR_IV_LENGTH
    CTR_IV_LENGTH   = 12,
#endif
#ifndef CCM_NONCE_LEN
    CCM_NONCE_LEN   = 11,
#endif
#ifndef CCM_TAG_LEN
    CCM_TAG_LEN     = 16,
#endif
#ifndef GCM_NONCE_LEN      /* micro_aes.h:108; any value but 12: J0 = GHASH(nonce) (micro_aes.c:1145-1149) */
    GCM_NONCE_LEN   = 12,
#endif
#ifndef GCM_TAG_LEN
    GCM_TAG_LEN     = 16,
#endif
#ifndef OCB_NONCE_LEN
    OCB_NONCE_LEN   = 12,
#endif
#ifndef OCB_TAG_LEN
    OCB_TAG_LEN     = 16,
#endif
    SIVGCM_NONCE_LEN = 12,
    SIVGCM_TAG_LEN  = 16,
#if EAX && !EAXP           /* (micro_aes.h:119: EAX' takes the nonce length as an argument and its mac has four bytes) */
#ifndef EAX_NONCE_LEN      /* micro_aes.h:120-121; -DEAX_NONCE_LEN=n (any, 0 too) / -DEAX_TAG_LEN=n (1..16) bind */
    EAX_NONCE_LEN   = 16,  /* AES_EAX_* to the general entry points below                                        */
#endif
#ifndef EAX_TAG_LEN
    EAX_TAG_LEN     = 16,
#endif
#endif
#if AES___ == 256 || AES___ == 192
    AES_KEYLENGTH   = AES___ / 8
#else
    AES_KEYLENGTH   = 16
#endif
};
typedef char uaes_ccm_lengths_ok[(CCM_NONCE_LEN >= 7 && CCM_NONCE_LEN <= 13 && CCM_TAG_LEN >= 4 && CCM_TAG_LEN <= 16 &&
                                  CCM_TAG_LEN % 2 == 0) ? 1 : -1];
typedef char uaes_ctr_lengths_ok[(CTR_IV_LENGTH >= 0 && CTR_IV_LENGTH <= 16) ? 1 : -1];
typedef char uaes_gcm_lengths_ok[(GCM_NONCE_LEN >= 1 && GCM_TAG_LEN >= 1 && GCM_TAG_LEN <= 16) ? 1 : -1];
typedef char uaes_ocb_lengths_ok[(OCB_NONCE_LEN >= 1 && OCB_NONCE_LEN <= 15 && OCB_TAG_LEN >= 1 && OCB_TAG_LEN <= 16) ? 1 : -1];

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

/* real functions behind OBJECT-like macros, so that `&AES_GCM_encrypt` / `&AES_CTR_encrypt` or a dispatch-table entry binds to
 * the lengths of this build as well as a direct call does                                              */
#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 199901L)
#define UAES_STATIC_INLINE static inline
#elif defined(__GNUC__)
#define UAES_STATIC_INLINE static __inline__ __attribute__((unused))
#else
#define UAES_STATIC_INLINE static
#endif

void AES_ECB_encrypt(const uint8_t *key,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
/* the same with padBlock's other two paddings (micro_aes.c:610-621): both ALWAYS append a
 * block, so crtxt must hold (ptextLen / 16 + 1) * 16 bytes                              */
void AES_ECB_encrypt_pkcs7(const uint8_t *key,
                           const void *pntxt, const size_t ptextLen, void *crtxt);
void AES_ECB_encrypt_iso7816(const uint8_t *key,
                             const void *pntxt, const size_t ptextLen, void *crtxt);
#if AES_PADDING == 1
#define AES_ECB_encrypt AES_ECB_encrypt_pkcs7
#elif AES_PADDING == 2
#define AES_ECB_encrypt AES_ECB_encrypt_iso7816
#endif
char AES_ECB_decrypt(const uint8_t *key,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);

void AES_CTR_encrypt(const uint8_t *key, const uint8_t *iv,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
void AES_CTR_decrypt(const uint8_t *key, const uint8_t *iv,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
/* PRESET_COUNTER is a compile-time switch of the CALLER's build in the reference: `iv` is then the
 * pre-initialised 16-byte counter block (bytes 9..15 = the 56-bit big-endian counter of incBlock,
 * micro_aes.c:421-427) -- the form in which a shard of a longer stream is encrypted.  Every library
 * exports both forms; a caller built with -DPRESET_COUNTER=1 is bound to these:                 */
void AES_CTR_encrypt_preset(const uint8_t *key, const uint8_t *counter16,
                            const void *pntxt, const size_t ptextLen, void *crtxt);
void AES_CTR_decrypt_preset(const uint8_t *key, const uint8_t *counter16,
                            const void *crtxt, const size_t crtxtLen, void *pntxt);
/* CTR_IV_LENGTH / CTR_START_VALUE other than 12 / 1 (micro_aes.h:98-99): counter block = iv[0..CTR_IV_LENGTH) ||
 * zeros with CTR_START_VALUE XORed in big-endian at its end (micro_aes.c:968-971).  Decrypt = encrypt (:986-990). */
void AES_CTR_encrypt_iv(const size_t ivLen, const size_t startValue, const uint8_t *key, const uint8_t *iv,
                        const void *pntxt, const size_t ptextLen, void *crtxt);
#if PRESET_COUNTER
#define AES_CTR_encrypt AES_CTR_encrypt_preset
#define AES_CTR_decrypt AES_CTR_decrypt_preset
#elif defined(CTR_IV_LENGTH) || defined(CTR_START_VALUE)
UAES_STATIC_INLINE void AES_CTR_encrypt_nl(const uint8_t *key, const uint8_t *iv,
                                        const void *pntxt, const size_t ptextLen, void *crtxt)
{
    AES_CTR_encrypt_iv(CTR_IV_LENGTH, CTR_START_VALUE, key, iv, pntxt, ptextLen, crtxt);
}
#define AES_CTR_encrypt AES_CTR_encrypt_nl
#define AES_CTR_decrypt AES_CTR_encrypt_nl
#endif

char AES_XTS_encrypt(const uint8_t *keys, const uint8_t *tweak,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_XTS_decrypt(const uint8_t *keys, const uint8_t *tweak,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);

void AES_GCM_encrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_GCM_decrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
/* GCM_NONCE_LEN / GCM_TAG_LEN are compile-time constants of the CALLER's build in the reference; with any nonce
 * length but 12 GCMsetup derives J0 = GHASH(nonce) (micro_aes.c:1145-1149), and GCM_TAG_LEN bytes of the tag are
 * appended / compared (:1178, :1204).  Every library exports the general entry points and a caller built with
 * -DGCM_NONCE_LEN=n and / or -DGCM_TAG_LEN=n is bound to them:                                                */
void AES_GCM_encrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_GCM_decrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *crtxt, const size_t crtxtLen, void *pntxt);
/* (the round-2 names: the same with a 16-byte tag) */
void AES_GCM_encrypt_ivlen(const size_t nonceLen, const uint8_t *key, const uint8_t *nonce,
                           const void *aData, const size_t aDataLen,
                           const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_GCM_decrypt_ivlen(const size_t nonceLen, const uint8_t *key, const uint8_t *nonce,
                           const void *aData, const size_t aDataLen,
                           const void *crtxt, const size_t crtxtLen, void *pntxt);

#if defined(GCM_NONCE_LEN) || defined(GCM_TAG_LEN)
UAES_STATIC_INLINE void AES_GCM_encrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *pntxt, const size_t ptextLen, void *crtxt)
{
    AES_GCM_encrypt_lens(GCM_NONCE_LEN, GCM_TAG_LEN, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
}
UAES_STATIC_INLINE char AES_GCM_decrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *crtxt, const size_t crtxtLen, void *pntxt)
{
    return AES_GCM_decrypt_lens(GCM_NONCE_LEN, GCM_TAG_LEN, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
}
#define AES_GCM_encrypt AES_GCM_encrypt_nl
#define AES_GCM_decrypt AES_GCM_decrypt_nl
#endif

char AES_CBC_encrypt(const uint8_t *key, const uint8_t iVec[16],
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_CBC_decrypt(const uint8_t *key, const uint8_t iVec[16],
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
/* CTS 0 (micro_aes.h:56): no stealing -- AES_CBC_encrypt pads its last chunk with padBlock like ECB (micro_aes.c:
 * 727-733; zeros behind a partial chunk, or PKCS#7 / ISO 7816-4 which always append: crtxt then holds
 * (ptextLen / 16 + 1) * 16 bytes), any length is accepted (:704-708), and AES_CBC_decrypt wants whole blocks
 * (:761, M_DATALENGTH_ERROR otherwise) and leaves the padding in place.  Every library exports both families:    */
char AES_CBC_encrypt_nocts(const uint8_t *key, const uint8_t iVec[16],
                           const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_CBC_encrypt_nocts_pkcs7(const uint8_t *key, const uint8_t iVec[16],
                                 const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_CBC_encrypt_nocts_iso7816(const uint8_t *key, const uint8_t iVec[16],
                                   const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_CBC_decrypt_nocts(const uint8_t *key, const uint8_t iVec[16],
                           const void *crtxt, const size_t crtxtLen, void *pntxt);
#if !CTS
#if AES_PADDING == 1
#define AES_CBC_encrypt AES_CBC_encrypt_nocts_pkcs7
#elif AES_PADDING == 2
#define AES_CBC_encrypt AES_CBC_encrypt_nocts_iso7816
#else
#define AES_CBC_encrypt AES_CBC_encrypt_nocts
#endif
#define AES_CBC_decrypt AES_CBC_decrypt_nocts
#endif

void AES_CFB_encrypt(const uint8_t *key, const uint8_t iVec[16],
                     const void *pntxt, const size_t ptextLen, void *crtxt);
void AES_CFB_decrypt(const uint8_t *key, const uint8_t iVec[16],
                     const void *crtxt, const size_t crtxtLen, void *pntxt);

void AES_OFB_encrypt(const uint8_t *key, const uint8_t iVec[16],
                     const void *pntxt, const size_t ptextLen, void *crtxt);
void AES_OFB_decrypt(const uint8_t *key, const uint8_t iVec[16],
                     const void *crtxt, const size_t crtxtLen, void *pntxt);

void AES_CCM_encrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_CCM_decrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);

/* CCM_NONCE_LEN (7..13) / CCM_TAG_LEN (even, 4..16), micro_aes.h:103-104: iv = { 14 - N, nonce, 0.. } (:1273), the
 * flags byte carries (T - 2) << 2 (:1229), T bytes of tag are appended / compared (:1281, :1308)                 */
void AES_CCM_encrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_CCM_decrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *crtxt, const size_t crtxtLen, void *pntxt);
#if defined(CCM_NONCE_LEN) || defined(CCM_TAG_LEN)
UAES_STATIC_INLINE void AES_CCM_encrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *pntxt, const size_t ptextLen, void *crtxt)
{
    AES_CCM_encrypt_lens(CCM_NONCE_LEN, CCM_TAG_LEN, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
}
UAES_STATIC_INLINE char AES_CCM_decrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *crtxt, const size_t crtxtLen, void *pntxt)
{
    return AES_CCM_decrypt_lens(CCM_NONCE_LEN, CCM_TAG_LEN, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
}
#define AES_CCM_encrypt AES_CCM_encrypt_nl
#define AES_CCM_decrypt AES_CCM_decrypt_nl
#endif

void AES_OCB_encrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_OCB_decrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
/* OCB_NONCE_LEN (1..15) / OCB_TAG_LEN (1..16), micro_aes.h:115-116: the nonce block of OCB_cipher (:1703-1709) */
void AES_OCB_encrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_OCB_decrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *crtxt, const size_t crtxtLen, void *pntxt);
#if defined(OCB_NONCE_LEN) || defined(OCB_TAG_LEN)
UAES_STATIC_INLINE void AES_OCB_encrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *pntxt, const size_t ptextLen, void *crtxt)
{
    AES_OCB_encrypt_lens(OCB_NONCE_LEN, OCB_TAG_LEN, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
}
UAES_STATIC_INLINE char AES_OCB_decrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *crtxt, const size_t crtxtLen, void *pntxt)
{
    return AES_OCB_decrypt_lens(OCB_NONCE_LEN, OCB_TAG_LEN, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
}
#define AES_OCB_encrypt AES_OCB_encrypt_nl
#define AES_OCB_decrypt AES_OCB_decrypt_nl
#endif

void GCM_SIV_encrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char GCM_SIV_decrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);

void AES_CMAC(const uint8_t *key,
              const void *data, const size_t dataSize, uint8_t mac[16]);

#if EAX && EAXP
/* EAX' (micro_aes.c:1523-1648 with EAXP 1; micro_aes.h:359-383): the AEAD of ANSI C12.22 / IEEE Std 1703.  No associated
 * data; the nonce (the datagram's cleartext header) has any length; mac = four bytes of N ^ C' appended at crtxt +
 * ptextLen; decrypt checks them before it writes (a forgery returns M_AUTHENTICATION_ERROR and leaves pntxt as it was).
 * AES_EAX_* are bound to the libraries' AES_EAXP_* symbols.  Minematsu, Lucks, Morita and Iwata (FSE 2013) forge EAX'
 * when nonce and text are both at most 16 bytes: the standard's own messages never are, and the mode belongs nowhere
 * else; such inputs are served all the same, as the reference serves them. */
void AES_EAXP_encrypt(const uint8_t *key, const uint8_t *nonce, const size_t nonceLen,
                      const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_EAXP_decrypt(const uint8_t *key, const uint8_t *nonce, const size_t nonceLen,
                      const void *crtxt, const size_t crtxtLen, void *pntxt);
#define AES_EAX_encrypt AES_EAXP_encrypt
#define AES_EAX_decrypt AES_EAXP_decrypt
#elif EAX
/* EAX (micro_aes.c:1560-1648): tag = N ^ H ^ C, EAX_TAG_LEN bytes appended at crtxt + ptextLen; decrypt checks the tag
 * before it writes (a forgery returns M_AUTHENTICATION_ERROR and leaves pntxt as it was) */
void AES_EAX_encrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_EAX_decrypt(const uint8_t *key, const uint8_t *nonce,
                     const void *aData, const size_t aDataLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
void AES_EAX_encrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_EAX_decrypt_lens(const size_t nonceLen, const size_t tagLen, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, const size_t aDataLen,
                          const void *crtxt, const size_t crtxtLen, void *pntxt);
#if defined(EAX_NONCE_LEN) || defined(EAX_TAG_LEN)
typedef char uaes_eax_lengths_ok[(EAX_TAG_LEN >= 1 && EAX_TAG_LEN <= 16) ? 1 : -1];
UAES_STATIC_INLINE void AES_EAX_encrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *pntxt, const size_t ptextLen, void *crtxt)
{
    AES_EAX_encrypt_lens(EAX_NONCE_LEN, EAX_TAG_LEN, key, nonce, aData, aDataLen, pntxt, ptextLen, crtxt);
}
UAES_STATIC_INLINE char AES_EAX_decrypt_nl(const uint8_t *key, const uint8_t *nonce,
                                           const void *aData, const size_t aDataLen,
                                           const void *crtxt, const size_t crtxtLen, void *pntxt)
{
    return AES_EAX_decrypt_lens(EAX_NONCE_LEN, EAX_TAG_LEN, key, nonce, aData, aDataLen, crtxt, crtxtLen, pntxt);
}
#define AES_EAX_encrypt AES_EAX_encrypt_nl
#define AES_EAX_decrypt AES_EAX_decrypt_nl
#endif
#endif

#if SIV
/* SIV, RFC 5297 (micro_aes.c:1323-1411): keys = K_s2v || K_ctr (AES_KEYLENGTH bytes each), iv = the synthesized IV;
 * decrypt returns M_AUTHENTICATION_ERROR on a mismatch */
void AES_SIV_encrypt(const uint8_t *keys,
                     const void *aData, const size_t aDataLen,
                     const void *pntxt, const size_t ptextLen,
                     uint8_t iv[16], void *crtxt);
char AES_SIV_decrypt(const uint8_t *keys, const uint8_t iv[16],
                     const void *aData, const size_t aDataLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
#endif

#if KWA
/* RFC 3394 (micro_aes.c:1829-1894): wrapped = secretLen + 8 bytes; M_DATALENGTH_ERROR unless secretLen is a multiple of 8
 * and at least 16 (unwrap: wrapLen at least 24), nothing written then.  unwrap returns M_AUTHENTICATION_ERROR when the
 * integrity value is not A6 x 8 and, like the reference, leaves what it computed in secret.  An engine failure makes
 * wrap return M_ENCRYPTION_ERROR and unwrap M_DECRYPTION_ERROR. */
char AES_KEY_wrap(const uint8_t *kek,
                  const void *secret, const size_t secretLen, void *wrapped);
char AES_KEY_unwrap(const uint8_t *kek,
                    const void *wrapped, const size_t wrapLen, void *secret);
#endif

#if FPE
/* FF1, SP 800-38G (micro_aes.c:2267-2347): a string of ptextLen characters of the alphabet to another such string, a NUL
 * behind it (crtxt holds ptextLen + 1 bytes).  Any failure -- a string shorter than the radix's minimum (6 for decimal)
 * or longer than 4096 characters (the reference takes any length), a character outside the alphabet, an engine failure
 * -- returns M_ENCRYPTION_ERROR / M_DECRYPTION_ERROR and leaves the output as it was. */
char AES_FPE_encrypt(const uint8_t *key, const uint8_t *tweak, const size_t tweakLen,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_FPE_decrypt(const uint8_t *key, const uint8_t *tweak, const size_t tweakLen,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
/* the alphabet is a compile-time choice of the CALLER's build in the reference; every library exports the general
 * entry points (alphabet = radix distinct characters, radix 2..256) and a caller built with -DCUSTOM_ALPHABET=n (1..9)
 * is bound to them with the ALPHABET and RADIX of its own micro_fpe.h, the file the reference's micro_aes.c includes */
char AES_FPE_encrypt_alpha(const char *alphabet, const size_t radix, const uint8_t *key, const uint8_t *tweak,
                           const size_t tweakLen, const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_FPE_decrypt_alpha(const char *alphabet, const size_t radix, const uint8_t *key, const uint8_t *tweak,
                           const size_t tweakLen, const void *crtxt, const size_t crtxtLen, void *pntxt);
#if CUSTOM_ALPHABET
#include "micro_fpe.h"
UAES_STATIC_INLINE char AES_FPE_encrypt_ca(const uint8_t *key, const uint8_t *tweak, const size_t tweakLen,
                                           const void *pntxt, const size_t ptextLen, void *crtxt)
{
    return AES_FPE_encrypt_alpha(ALPHABET, RADIX, key, tweak, tweakLen, pntxt, ptextLen, crtxt);
}
UAES_STATIC_INLINE char AES_FPE_decrypt_ca(const uint8_t *key, const uint8_t *tweak, const size_t tweakLen,
                                           const void *crtxt, const size_t crtxtLen, void *pntxt)
{
    return AES_FPE_decrypt_alpha(ALPHABET, RADIX, key, tweak, tweakLen, crtxt, crtxtLen, pntxt);
}
#define AES_FPE_encrypt AES_FPE_encrypt_ca
#define AES_FPE_decrypt AES_FPE_decrypt_ca
#endif
/* FF3-1, SP 800-38G revision 1 (micro_aes.c:2150-2248): what the reference's AES_FPE_* are when it is built with FF_X 3,
 * under names of their own -- the same parameter list (no tweakLen: the tweak is FF3_TWEAK_LEN bytes), the decimal
 * alphabet, a NUL behind the output.  Any failure -- a string shorter than 6 or longer than 56 characters, a character
 * that is no digit, an engine failure -- returns M_ENCRYPTION_ERROR / M_DECRYPTION_ERROR and leaves the output as it
 * was.  The _alpha pair takes the alphabet (radix distinct characters, radix 2..256; the length limits follow it). */
enum { FF3_TWEAK_LEN = 7 };
char AES_FF3_encrypt(const uint8_t *key, const uint8_t *tweak,
                     const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_FF3_decrypt(const uint8_t *key, const uint8_t *tweak,
                     const void *crtxt, const size_t crtxtLen, void *pntxt);
char AES_FF3_encrypt_alpha(const char *alphabet, const size_t radix, const uint8_t *key, const uint8_t *tweak,
                           const void *pntxt, const size_t ptextLen, void *crtxt);
char AES_FF3_decrypt_alpha(const char *alphabet, const size_t radix, const uint8_t *key, const uint8_t *tweak,
                           const void *crtxt, const size_t crtxtLen, void *pntxt);
#endif

#if POLY1305
/* keys = k (AES_KEYLENGTH bytes) || r (16 bytes); mac = Poly1305-AES of data under nonce (micro_aes.h:444-450) */
void AES_Poly1305(const uint8_t *keys, const uint8_t nonce[16],
                  const void *data, const size_t dataSize, uint8_t mac[16]);
#endif

/* Not in the reference: what happens when a `void` function above cannot do its work
 * (no usable HIP device, an allocation or launch failure -- there is no CPU path).  The
 * default handler prints the reason and abort()s; install another to unwind instead.
 * Returns the previous handler (NULL = the default).  fn = API name, rc = engine code
 * (include/uaes_hip.h), msg = uaes_last_error().                                      */
typedef void (*uaes_failure_handler)(const char *fn, int rc, const char *msg);
uaes_failure_handler uaes_compat_set_failure_handler(uaes_failure_handler h);

/* Not in the reference either: DEVICE pointers are accepted wherever the reference takes a buffer.  A call first waits
 * for the work the caller may have in flight on the default stream; a caller that produces its data on a stream of
 * its own (hipStreamNonBlocking streams do not synchronise with the default one) names that stream here, per thread
 * (a hipStream_t; NULL = the default stream again).  Long HOST buffers can be spread over several GPUs without a
 * change in the caller: environment variable UAES_DEVICES=all | 0,1,... (include/uaes_hip.h, uaes_set_devices).   */
void uaes_compat_set_producer_stream(void *stream);

#ifdef __cplusplus
}
#endif

enum function_result_codes
{
    M_ENCRYPTION_ERROR     = 0x1E,
    M_DECRYPTION_ERROR     = 0x1D,
    M_AUTHENTICATION_ERROR = 0x1A,
    M_DATALENGTH_ERROR     = 0x1L,
    M_RESULT_SUCCESS       = 0
};

#endif /* MICRO_AES_H_ */
