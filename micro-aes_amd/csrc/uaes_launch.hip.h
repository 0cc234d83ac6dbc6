/*
 * uaes_launch.hip.h -- the host-side plumbing every kernel file shares, between its extern "C" entry points and the
 * launch itself: the stream cast, the key-size and bool dispatch, the one launch helper, the CU count and the
 * per-thread state of a synchronous call (ticket, done word).  Host code only.
 */
#ifndef UAES_LAUNCH_HIP_H_
#define UAES_LAUNCH_HIP_H_

#include <hip/hip_runtime.h>
#include <type_traits>
#include "uaes_device.h"
#include "uaes_plan.h"

/* ---- completion ticket riding on a kernel (uaes_device.h: uaesk_done; device side: ticket_release) ---- */
uaesk_done uaesk_ticket_take();                     /* the calling host thread's armed ticket (cleared), uaes_kernels.hip */
void uaesk_ticket_unused();
unsigned *uaesk_done_word_take();                    /* the armed zero-between-calls word (cleared), uaes_kernels.hip */
bool uaesk_gcm_fold_on();                             /* UAES_GCM_FOLD is not 0 (uaes_kernels.hip) */
bool uaesk_arr_on(int id);                            /* the arrangement is not switched off (uaes_kernels.hip) */
hipError_t uaesk_want_lds(const void *kern, unsigned bytes);   /* dynamic-LDS attribute, set once per (kernel, device) */
int uaesk_cus();                                      /* CUs of the current device, cached per ordinal; 0: no device to ask */

/* a multi-launch routine takes the ticket at its entry, so that the single-launch building blocks it calls do not
 * pick it up in the middle of the sequence, and hands it to the one path that is a single launch (use()); if no
 * such path was taken the host layer is told so (uaesk_ticket_disarm() = 1) and sends k_ticket itself          */
struct TicketScope {
    uaesk_done d;
    bool used;
    TicketScope() : d(uaesk_ticket_take()), used(false) {}
    ~TicketScope() { if (d.flag && !used) uaesk_ticket_unused(); }
    const uaesk_done &use() { used = true; return d; }
};

static inline hipStream_t S(void *s) { return (hipStream_t)s; }

/* the CU count the planners size their grids by; no device: the table of a 256-CU MI355X */
static inline unsigned uaesk_cus_or_256()
{
    const int cus = uaesk_cus();
    return cus ? (unsigned)cus : 256u;
}

/* The launch shape of every row batch (sixteen lanes per record, four records per wave, a grid-stride loop over the
 * records): 64 records per 16-wave workgroup.  Few records -- while such workgroups would fill at most half the CUs --
 * run in 4-wave workgroups instead, so that they spread over four times as many CUs: every record is a serial chain
 * that its row walks alone, so a batch is only as fast as the number of SIMDs it reaches (profiles/HISTORY.md,
 * "sixteen lanes per message", has the measurements).  The grid is capped at the CU count and the kernels stride
 * beyond it; no records still is a grid of 1. */
struct RowShape { unsigned grid, wg; };
constexpr unsigned UAESK_ROW_WG = 1024u;             /* = UAES_WG, the row kernels' launch bound (uaes_aes.hip.h asserts it) */
static inline RowShape uaesk_row_shape(unsigned long long nrec)
{
    const unsigned cus = uaesk_cus_or_256();
    const unsigned wg = (nrec + 63) / 64 * 2 <= cus ? 256u : UAESK_ROW_WG;
    const unsigned long long want = (nrec + wg / 16 - 1) / (wg / 16);
    return RowShape{ (unsigned)(want < cus ? (want ? want : 1) : cus), wg };
}

/* the plan of a row batch that is one launch of that shape: steps = threads per workgroup */
static inline void uaesk_row_plan(int arrangement, unsigned long long nrec, uaes_plan *p)
{
    const RowShape s = uaesk_row_shape(nrec);
    p->arrangement = arrangement;
    p->launches = 1;
    p->grid = s.grid;
    p->steps = s.wg;
}

/* the row kernels' A4: both texts and the record size are 4-byte aligned, so every record is */
static inline bool uaesk_rows_a4(const void *in, const void *out, size_t rec_bytes)
{
    return ((((uintptr_t)in) | ((uintptr_t)out)) & 3u) == 0 && rec_bytes % 4 == 0;
}

#define DISPATCH_NR(nr, CALL)                         \
    switch (nr) {                                     \
    case 10: { constexpr int NR = 10; CALL; } break;  \
    case 12: { constexpr int NR = 12; CALL; } break;  \
    case 14: { constexpr int NR = 14; CALL; } break;  \
    default: return (int)hipErrorInvalidValue;        \
    }

/* a run-time bool as a template argument: with_bool(decrypt, [&](auto D) { constexpr bool DEC = decltype(D)::value; ... }) */
template <typename F>
static inline auto with_bool(bool b, F f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

/* one launch: the kernel's dynamic-LDS attribute (a table hit after the first time; a kernel without dynamic LDS needs
 * none; one that asks for less than 64 KiB gets it all the same, which costs that table hit and nothing else), the
 * launch with every argument converted to the kernel's own parameter type, the launch's error.  The attribute comes
 * after whatever the caller did before, taking the call's ticket included: a launch that fails here or in the runtime
 * leaves the ticket taken and unsent, which the host layer handles as any failed launch.
 * static_cast<P> takes what an implicit conversion would and also void * to T * and a narrowing integer, so that two
 * arguments of one kind written in the wrong order compile: the order at a call site is checked against the kernel's
 * parameter list by reading, as with the macro it replaces. */
template <typename... P, typename... A>
static inline int uaesk_launch(void (*kern)(P...), dim3 grid, dim3 wg, unsigned lds, hipStream_t st, A &&...args)
{
    const hipError_t e = lds ? uaesk_want_lds((const void *)kern, lds) : hipSuccess;
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, grid, wg, lds, st, static_cast<P>(args)...);
    return (int)hipGetLastError();
}

#endif /* UAES_LAUNCH_HIP_H_ */
