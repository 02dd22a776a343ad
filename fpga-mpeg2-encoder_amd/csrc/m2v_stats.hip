// m2v_stats.hip — option "stats", host side: per-picture records (include/m2v_mi355x.h, m2v_picture_stats) made on the device while a chunk is
// encoded.  Everything they need is there anyway: the 4:4:4 source, the reconstruction k_mb writes (with the option on, of EVERY
// picture: plan_chunk), the info word and the bit count of every macroblock.
//
// The kernels (m2v_stats_kernels.hpp, launched from m2v_launch.hip):
//   k_picstat      behind the k_mb launches of a GOP step, on their stream: squared error of the step's pictures, source against
//                  reconstruction, into the records' three 64-bit sums.  The slot it reads is rewritten two steps later, and plain
//                  stream order keeps it ahead of that.
//   k_picstat_mb   behind the chunk's scans (k_slice_scan makes the bit counts): one block per picture writes the rest of its record.
//
// The records then travel to pinned memory of the chunk's stage in front of its control word, and reach the handle's queue where the
// host has waited for that chunk anyway.  No wait is added anywhere.  Integers only: a record depends on no launch shape.
#include "m2v_host.hpp"

static_assert(sizeof(m2v_picture_stat) == 64, "the record of include/m2v_mi355x.h is 64 bytes");

namespace m2v {

void stats_begin_chunk(m2v_enc *e, hipStream_t s, size_t nf)
{
    e->d_pstat.recorded = false;
    e->d_pstat.ensure(nf);
    HIPCHK(hipMemsetAsync(e->d_pstat.p, 0, nf * sizeof(m2v_picture_stat), s));
}

void stats_finish_chunk(m2v_enc *e, hipStream_t s)
{
    const size_t nf = e->plan_nf;
    m2v_enc::HostStage &h = e->st();
    launch_picstat_mb(e, s, nf);
    if (h.h_pstat_cap < nf) {           // (the stage is free: its previous chunk has completed)
        if (h.h_pstat) (void)hipHostFree(h.h_pstat);
        h.h_pstat = nullptr; h.h_pstat_cap = 0;
        HIPCHK(hipHostMalloc((void **)&h.h_pstat, nf * sizeof(m2v_picture_stat)));
        h.h_pstat_cap = nf;
    }
    HIPCHK(hipMemcpyAsync(h.h_pstat, e->d_pstat.p, nf * sizeof(m2v_picture_stat), hipMemcpyDeviceToHost, s));
    h.nstat = nf;
}

}  // namespace m2v

extern "C" long long m2v_picture_stats(m2v_enc *e, m2v_picture_stat *dst, size_t cap)
{
    if (!e) return M2V_E_PARAM;
    return (long long)e->pstat_q.pop(dst, cap);
}
