/*
 * bsw_fmi_launch.h -- how the last seeding call of an index was launched (additive to ABI
 * version 8: BSW_FMI_LAUNCH_API; bsw_fmi.h and its symbol list are unchanged).
 *
 * bsw_mem_collect_intv(_device) splits a batch into several launches of the SMEM kernel so that
 * the walk's two scratch vectors (2 x (max_len + 1) entries per read) stay within a budget:
 * 16 GiB, or BSW_SMEM_SCRATCH_MB MiB when that environment variable is set (read once per call;
 * values below 1 count as 1).  A launch holds at least 64 reads whatever the budget.  The
 * variable exists for tests: with it the chunked path (read index n0 + t, per-chunk stride, a last
 * chunk shorter than a wave) runs on a few hundred reads instead of a 16 GiB allocation.
 */
#ifndef BSW_FMI_LAUNCH_H
#define BSW_FMI_LAUNCH_H

#include <stdint.h>
#include "bsw_fmi.h"

#define BSW_FMI_LAUNCH_API 1

#ifdef __cplusplus
extern "C" {
#endif

/* Of the last seeding call on `fmi` (0, 0 before the first): the number of SMEM kernel launches and
 * the size of one scratch entry -- 16 (narrow index, or wide with packed entries) or 32 (wide with
 * plain entries: BSW_FMI_PLAIN_ENT, max_len = BSW_MAX_LEN, or an index past the packed form). */
int  bsw_fmi_last_launch(const bsw_fmi_t *fmi, int32_t *launches, int32_t *entry_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BSW_FMI_LAUNCH_H */
