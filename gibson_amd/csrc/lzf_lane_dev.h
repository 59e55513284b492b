/*
 * lzf_lane_dev.h -- what the lane generation's product file (lzf_lane.hip) and
 * its diagnostic forms (lzf_lane_diag.hip, diagnostic library only) share: the
 * size classes of the diagnostic cand kernels, the residency cap of the
 * one-lane-per-value launches, the debug-build site counters, and the hooks by
 * which the product launcher hands a launch to a diagnostic form.
 */
#ifndef GIBSON_AMD_LZF_LANE_DEV_H
#define GIBSON_AMD_LZF_LANE_DEV_H

#include <stdlib.h>
#include <string.h>

#include "lzf_dev.h"

/* cand word (u16 per position, LzfLaneScratch::cand): bits 0-12 off = p - q - 1,
 * bits 13-15 the agreement code (dv_code, lzf_dev.h) */

#define KS_MAXN     4096u         /* small class: 12-bit bucket, 4-bit identity, positions + 1 fit 12 bits */
#define KS8_MAXN    8192u         /* small class, 8 KiB: 13-bit bucket, 3-bit identity, positions + 1 fit 13 bits */
#define KR_MAXN     16384u        /* ring class, bytes staged whole */
#define KR64_MAXN   65536u        /* ring class, bytes streamed */
#define KM_MAXN     65536u        /* mid class: positions + 1 fit 16 bits */
#define KW_MAXN     KS_MAXN       /* wave-form parse: the small class */

/* Residency cap for the one-lane-per-value kernels: each lane streams its own
 * value, so the lines in use grow with the lanes in flight; past what the
 * XCD's L2 holds every access refetches its line.  Capping the blocks per CU
 * (through the LDS reservation of the launch) trades latency hiding for
 * L2 hits.  0 = no cap. */
static inline size_t lane_lds_for(const char *env, uint32_t dflt_blocks_per_cu)
{
    const char *e = getenv(env);
    const uint32_t b = e ? (uint32_t)atoi(e) : dflt_blocks_per_cu;
    if (b == 0u) return 0;
    size_t lds = (160u * 1024u) / b;
    if (lds > 64u * 1024u) lds = 64u * 1024u;
    return lds - 256u;
}

/* Debug builds only (-DK2_COUNT_SITES, -DK2_WAVE_SITES, -DKW_PHASES through
 * tools/build_variant.sh): event counts of the parse kernels, summed over all
 * lanes.  Each of the two files counts in its own copy (device symbols do not
 * cross files); lzf_gpu_debug_sites (lzf_lane.hip) reports their sum. */
#if defined(K2_COUNT_SITES) || defined(KW_PHASES) || defined(K2_WAVE_SITES)
static __device__ unsigned long long k2_sites[16];
static int k2_sites_add(unsigned long long *out16, int reset)
{
    unsigned long long t[16];
    hipError_t e = hipMemcpyFromSymbol(t, HIP_SYMBOL(k2_sites), sizeof(t));
    for (int i = 0; i < 16 && e == hipSuccess; i++) out16[i] += t[i];
    if (e == hipSuccess && reset) {
        unsigned long long z[16] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(k2_sites), z, sizeof(z));
    }
    return e == hipSuccess ? 0 : -2;
}
#endif
#ifdef K2_COUNT_SITES
#define K2_SITE(i) atomicAdd(&k2_sites[i], 1ull)
#else
#define K2_SITE(i) ((void)0)
#endif

/* The diagnostic forms, selected per launch by the LZF_GPU_* variables of
 * INTEGRATION.md §5.  The product library has none of them: its hooks are
 * constants, and the launcher's calls fold away. */
#ifdef LZF_DIAG
bool lzf_lane_diag_cand_small(void);                 /* LZF_GPU_CAND=small */
bool lzf_lane_diag_supported(uint32_t max_len);      /* value sizes the small / ring / mid classes take */
/* kernel 1 by the small, ring or mid class when LZF_GPU_CAND=small: true when it launched */
bool lzf_lane_diag_cand(const LzfBatch &c, const LzfLaneScratch &sc, uint32_t max_len, hipStream_t s);
/* kernel 2 by the wave form when LZF_GPU_LANE_PARSE=w (small class): true when it launched */
bool lzf_lane_diag_parse(const LzfBatch &c, const LzfLaneScratch &sc, uint32_t max_len, hipStream_t s);
int lzf_lane_diag_sites(unsigned long long *out16, int reset);
#else
static inline bool lzf_lane_diag_cand_small(void) { return false; }
static inline bool lzf_lane_diag_supported(uint32_t) { return false; }
static inline bool lzf_lane_diag_cand(const LzfBatch &, const LzfLaneScratch &, uint32_t, hipStream_t) { return false; }
static inline bool lzf_lane_diag_parse(const LzfBatch &, const LzfLaneScratch &, uint32_t, hipStream_t) { return false; }
static inline int lzf_lane_diag_sites(unsigned long long *, int) { return 0; }
#endif

#endif
