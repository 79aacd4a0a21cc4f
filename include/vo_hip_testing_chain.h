/* Test- and tool-only entry points of libvo_hip.so for the chained GN loop.
 * Not part of the product surface (vo_hip.h).  They sit beside vo_hip_testing.h in a header of
 * their own: tests/test_abi.py pins that header's list of functions. */
#ifndef VO_HIP_TESTING_CHAIN_H
#define VO_HIP_TESTING_CHAIN_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test switch: on != 0 keeps vo_ba_run / vo_ba_run_async of this context on the split sequence
 * (a K1 launch, then the fused reduction + solve launch, per iteration).  By default a run of
 * two or more iterations of a window that qualifies (one rank, fused full-layout solve, six-chunk
 * wave plan, segments + 2 <= CUs, no kernel profiling) enqueues one stand-alone K1, then solve
 * launches that each carry the next iteration's K1 behind a pose gate, then one plain fused
 * launch.  Same kernels' arithmetic: the GPU tests compare the two bitwise.  Takes effect at the
 * next run. */
int vo_ba_testing_no_chain(vo_ctx* ctx, int on);

/* Whether the context's last vo_ba_run / vo_ba_run_async was chained (*chained 0 / 1) and how
 * many K1 and solve launches its iterations made (*launches: 2 k split, k + 1 chained; the
 * read-out's launches behind the last iteration are not counted; nor is the prior's kernel that a
 * session set up with a pose prior or pose factors enqueues behind every K1 launch, so such a
 * session reports 2 k for the 3 k kernels of its iterations).  Either pointer may be NULL. */
int vo_ba_testing_last_run(vo_ctx* ctx, int* chained, int* launches);

/* Tool switch: replicas of the publish word the chained K1 workgroups poll (1: one word; 8: one
 * of eight words on lines of their own, chosen by workgroup index; 0: the build's default). */
int vo_ba_testing_chain_poll(vo_ctx* ctx, int replicas);

/* Tool entry, stamped builds (VO_BA_STAMPS): on != 0 lets this context's runs chain although
 * stamps are on, each K1 workgroup of a chained launch recording s_memrealtime at its start,
 * prefix done, gate passed and end.  out (may be NULL): the last chained launch's values,
 * [solver published, launch start | four per K1 workgroup], at most n; returns how many (0 in a
 * product build). */
int vo_ba_testing_chain_stamps(vo_ctx* ctx, int on, uint64_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* VO_HIP_TESTING_CHAIN_H */
