// m2v_desc.hip — what the stream says about itself, host side.  The module hard-wires its sequence headers (RTL:2598-2617: 24 frames per
// second, square samples, 4 Mbit/s, no vbv size, BT.470BG / BT.601 colour) and counts its time code at 24 frames per second
// (RTL:2685-2698); here the caller says otherwise (m2v_set_stream_desc).  The stream stays a legal one - the fields are ISO/IEC 13818-2's,
// every value inside its table - and nothing but the header bytes depends on it.  Not the module's behaviour.
//
//   the writers            write_sequence_headers and write_frame_headers (m2v_kernels.hpp) take the values instead of literals: a packed
//                          SeqDesc (m2v_types.hpp), passed by value to k_assemble.  There is one code path: the module's stream is these
//                          functions with seq_desc_module().  k_mb is untouched.
//   repeat_headers         the same 34 bytes in front of the group_start_code of every GOP after the first (ISO 6.1.1.6), whatever started
//                          the GOP.  k_frame_scan leaves the room - its one new argument - and the thread of k_assemble that writes a
//                          frame's headers writes them at frame_off[f] - 34.  A GOP's size (m2v_gop_stat, the cap) does not count them.
//   the time code          time_code (m2v_types.hpp), one __host__ __device__ definition: k_assemble prints it, m2v_time_code exports it.
//
// No launch, buffer, wait or copy is added anywhere; a setting equal to the module's counts as none.
#include "m2v_host.hpp"

static_assert(sizeof(m2v_stream_desc) == 48, "the structure of include/m2v_mi355x.h is 48 bytes");
static_assert(sizeof(SeqDesc) == 16, "a few dwords by value");

namespace m2v {

static const m2v_stream_desc kModuleDesc = {2, 1, 10000, 0, 1, 5, 5, 5, 0, 0, 0, 0};

// the first field out of range, nullptr if none
static const char *desc_fault(const m2v_stream_desc &d)
{
    if (d.frame_rate_code < 1 || d.frame_rate_code > 8) return "frame_rate_code is 1..8";
    if (d.aspect_ratio_information < 1 || d.aspect_ratio_information > 4) return "aspect_ratio_information is 1..4";
    if (d.bit_rate_400 < 1 || d.bit_rate_400 > 0x3FFFFFFFu) return "bit_rate_400 is 1..2^30 - 1";
    if (d.vbv_buffer_size_16k > 0x3FFFFu) return "vbv_buffer_size_16k is 0..2^18 - 1";
    if (d.video_format > 5) return "video_format is 0..5";
    if (d.colour_primaries < 1 || d.colour_primaries > 255) return "colour_primaries is 1..255";
    if (d.transfer_characteristics < 1 || d.transfer_characteristics > 255) return "transfer_characteristics is 1..255";
    if (d.matrix_coefficients < 1 || d.matrix_coefficients > 255) return "matrix_coefficients is 1..255";
    if ((d.display_width == 0) != (d.display_height == 0)) return "display_width and display_height are both 0 or both 1..16383";
    if (d.display_width > 16383 || d.display_height > 16383) return "display_width and display_height are both 0 or both 1..16383";
    if (d.repeat_headers > 1) return "repeat_headers is 0 or 1";
    if (d.reserved != 0) return "reserved is 0";
    return nullptr;
}

SeqDesc pack_desc(const m2v_stream_desc &d)
{
    return SeqDesc{d.frame_rate_code | d.aspect_ratio_information << 4 | d.video_format << 8 | d.repeat_headers << 11 | d.vbv_buffer_size_16k << 12,
                   d.bit_rate_400, d.colour_primaries | d.transfer_characteristics << 8 | d.matrix_coefficients << 16,
                   d.display_width | d.display_height << 16};
}

}  // namespace m2v

extern "C" {

void m2v_stream_desc_module(m2v_stream_desc *d)
{
    if (d) *d = kModuleDesc;
}

int m2v_set_stream_desc(m2v_enc *e, const m2v_stream_desc *d)
{
    if (!e) return M2V_E_PARAM;
    if (in_progress(e, "m2v_set_stream_desc", "the description is sampled when a sequence starts")) return M2V_E_STATE;
    if (!d) { e->set.desc_set = false; return M2V_OK; }
    if (const char *why = desc_fault(*d)) {
        e->set_err("m2v_set_stream_desc: %s (the previous setting stays)", why);
        return M2V_E_PARAM;
    }
    e->set.desc = *d;
    e->set.desc_set = memcmp(d, &kModuleDesc, sizeof *d) != 0;
    return M2V_OK;
}

int m2v_frame_rate_code(uint32_t num, uint32_t den)
{
    // table 6-4: 24000/1001, 24, 25, 30000/1001, 30, 50, 60000/1001, 60
    static const uint32_t N[8] = {24000, 24, 25, 30000, 30, 50, 60000, 60}, D[8] = {1001, 1, 1, 1001, 1, 1, 1001, 1};
    if (!num || !den) return M2V_E_PARAM;
    for (int k = 0; k < 8; ++k)
        if ((unsigned long long)num * D[k] == (unsigned long long)den * N[k]) return k + 1;
    return M2V_E_PARAM;
}

int m2v_time_code(uint32_t frame_rate_code, uint32_t n, uint8_t out[4])
{
    if (frame_rate_code < 1 || frame_rate_code > 8 || !out) return M2V_E_PARAM;
    const uint32_t v = time_code(time_code_rate(frame_rate_code), n);
    out[0] = (uint8_t)(v >> 24); out[1] = (uint8_t)(v >> 16); out[2] = (uint8_t)(v >> 8); out[3] = (uint8_t)v;
    return M2V_OK;
}

}  // extern "C"
