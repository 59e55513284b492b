/*
 * gb_policy.h -- the store policy of gbSingleSet that the host call sites
 * (gb_batch.c) and the device SET path (lzf_store.hip) share, written once.
 * Plain C; under hipcc the functions are callable from kernels too.
 */
#ifndef GIBSON_AMD_GB_POLICY_H
#define GIBSON_AMD_GB_POLICY_H

#include <stdint.h>

#ifdef __HIPCC__
#define GB_POLICY_FN static __host__ __device__ inline
#else
#define GB_POLICY_FN static inline
#endif

/* out_len of src/query.c:384-391: size_t needcompr = vlen - 4, passed as
 * unsigned int, so a value of fewer than 4 bytes gets a wrapped, huge cap.
 * No LZF stream of vlen bytes exceeds vlen + vlen/32 + 1 bytes, so a cap
 * past vlen + vlen/16 + 8 decides exactly like the wrapped one. */
GB_POLICY_FN uint32_t gb_needcompr(uint32_t vlen)
{
    const uint32_t c = (uint32_t)(vlen - 4u), most = vlen + vlen / 16u + 8u;
    return c < most ? c : most;
}

#endif
