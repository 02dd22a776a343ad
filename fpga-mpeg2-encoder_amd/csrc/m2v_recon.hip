// m2v_recon.hip — m2v_set_recon_out, host side: every coded picture of a resident sequence as a plain 4:2:0 frame in a device buffer of
// the caller's (include/m2v_mi355x.h).  Everything it needs is there anyway once every picture keeps its reconstruction, which option
// "stats" already taught plan_chunk: with a buffer sampled, a picture has a slot if followed || stats || recon, and
//
//   k_recon_out (m2v_recon_kernels.hpp, launched from m2v_launch.hip) runs behind the k_mb launches of a GOP step, on their stream -
//               where k_picstat runs - and writes the step's pictures, all planes in one launch, to frame FrameJob::n of the buffer.
//               The slot it reads is rewritten two steps later, and plain stream order keeps it ahead of that.  A GOP that option
//               "gop_bytes_max" codes again is written again behind its redo steps: the frames of its final level stay.
//
// No wait, no buffer and no copy is added anywhere; k_mb is untouched.  With no buffer set nothing here is reached.
#include "m2v_host.hpp"

namespace m2v {

// bytes of one frame k_recon_out writes: the size set (m2v_set_frame_size: the source's size while the sequence pads its frames, and the
// coded size where it is whole macroblocks), else the coded picture of xs x ys macroblocks
size_t recon_frame_bytes(const m2v_enc *e, uint32_t xs, uint32_t ys)
{
    const Geom g = make_geom(e, xs, ys);
    const size_t w = e->set.size.w ? (size_t)e->set.size.w : (size_t)g.W, h = e->set.size.w ? (size_t)e->set.size.h : (size_t)g.H;
    return w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2);
}

}  // namespace m2v

extern "C" int m2v_set_recon_out(m2v_enc *e, void *d_dst, size_t cap, int layout)
{
    if (!e) return M2V_E_PARAM;
    if (in_progress(e, "m2v_set_recon_out", "the buffer is sampled when a sequence starts")) return M2V_E_STATE;
    if (d_dst && !layout420_ok(layout)) { e->set_err("m2v_set_recon_out: unknown layout %d", layout); return M2V_E_PARAM; }
    // (what the last sequence sampled goes with the old setting)
    e->seq.recon = m2v_enc::ReconDst{};
    e->set.recon = m2v_enc::ReconDst{};
    if (d_dst) { e->set.recon.p = (uint8_t *)d_dst; e->set.recon.cap = cap; e->set.recon.layout = layout; }
    return M2V_OK;
}
