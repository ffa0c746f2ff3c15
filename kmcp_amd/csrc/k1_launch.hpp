// k1_launch.hpp — the K1 kernel families behind launch_k1 (k1_kmers.hip).  A kernel is launched from the file that defines it (no
// relocatable device code), so each family file offers one host launcher per plan form it serves: the launches of that form, in order,
// each noted in the log.  Everything was decided by the plan (k1_plan.hpp): `a` is complete and no launcher looks at the batch again.
#pragma once
#include <hip/hip_runtime.h>

#include "k1_plan.hpp"
#include "kernels.hpp"

namespace kmcpg {

// What a launch leaves in the log (kmcpg_last_k1_launches).  Every templated kernel is launched by a function template of the same
// parameters that writes them itself, so a record cannot name another instantiation than the one that ran.
void k1_note(K1Log* log, int kernel, int p0, int p1, unsigned grid, unsigned block, size_t lds);

// k1_reads.hip
void launch_k1_short(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);      // k1_kmers<mode>
void launch_k1_wg(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);         // k1_kmers_wg<mode>
void launch_k1_wg_global(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);  // k1_kmers_wg_global
void launch_k1_seg_hash(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);   // k1_seg_hash alone (launch_k1_seg_pack follows)
// k1_windows.hip
void launch_k1_windows_wave(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);  // k1_windows_wave<mode>
void launch_k1_windows_roll(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);  // k1_windows_roll<wsz, waves>, k1_windows_wave<2> behind it
// k1_seg.hip
void launch_k1_seg_pack(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);   // k1_seg_pack
void launch_k1_seg_roll(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);   // k1_seg_roll, k1_seg_pack
void launch_k1_seg_roll2(const K1Args& a, const K1Plan& p, hipStream_t st, K1Log* log);  // k1_seg_roll2 (+ k_mark_exc, k_unpack2_list, k1_seg_roll over the list), k1_seg_pack
// k1_win_once.hip
void launch_k1_win_once(const K1Args& a, const K1Plan& p, const K1WinOnce& wo, hipStream_t st, K1Log* log);  // k1_win_hash / scan / rank / gather

}  // namespace kmcpg
