/*
 * m2v_container.h — stream-level conveniences around the encoder's output (libm2v_container.so, plain C++,
 * no GPU): a structural scan of the elementary stream (sizes / types per picture: the numbers the reference's
 * README:735-768 quotes per clip) and MPEG-2 Program Stream / Transport Stream multiplexers so that the `.m2v`
 * the module produces (SIM/tb_mpeg2encoder.v:260-262 writes the bare elementary stream) can be played and muxed
 * with audio by ordinary tools.  SURVEY.md 8(f4): usefulness beyond parity; nothing here touches the encoded bits.
 *
 * All functions return 0 / a count on success and a negative M2VC_E_* code on failure.  Buffers are caller owned.
 */
#ifndef M2V_CONTAINER_H
#define M2V_CONTAINER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    M2VC_OK         = 0,
    M2VC_E_PARAM    = -1,
    M2VC_E_SYNTAX   = -2,   /* not an MPEG-2 video elementary stream as this encoder writes it */
    M2VC_E_OVERFLOW = -3    /* output buffer / picture table too small */
};

typedef struct {
    uint32_t width, height;          /* sequence_header horizontal/vertical_size_value (RTL:2600-2603) */
    uint32_t frame_rate_code;        /* ISO/IEC 13818-2 table 6-4; the RTL writes 2 = 24 fps (RTL:2598-2617) */
    uint32_t aspect_ratio_code;
    uint32_t bit_rate_400;           /* bit_rate_value, units of 400 bit/s (0x3FFFF = variable) */
    uint32_t pictures, i_pictures, p_pictures, gops, slices;
    uint64_t bytes;                  /* stream length without the zero padding after sequence_end_code */
    uint64_t padding_bytes;          /* zero bytes after sequence_end_code (RTL:2932-2937 pads to 32-byte words) */
    int      has_sequence_end;
} m2vc_stream_info;

typedef struct {
    uint64_t offset;                 /* byte offset of the picture's first start code (GOP header if one precedes it; a sequence header repeated in front of that GOP header if there is one) */
    uint64_t bytes;                  /* up to the next picture / sequence end */
    uint32_t coding_type;            /* 1 = I, 2 = P */
    uint32_t temporal_reference;
    uint32_t gop_start;              /* 1 if a group_of_pictures_header precedes the picture */
    uint32_t slices;
} m2vc_picture;

/* frames per second of a frame_rate_code as a rational (0/1 for reserved codes) */
int m2vc_frame_rate(uint32_t frame_rate_code, uint32_t *num, uint32_t *den);

/*
 * Structural scan.  `pics` may be NULL (count only); otherwise up to `cap` entries are filled and *npics receives
 * the number of pictures in the stream (M2VC_E_OVERFLOW if cap was too small, the first cap entries are valid).
 */
int m2vc_scan(const uint8_t *es, size_t es_bytes, m2vc_stream_info *info, m2vc_picture *pics, size_t cap,
              size_t *npics);

/*
 * Both multiplexers are for FILE PLAYBACK: SCR / PCR advance with the byte position at a constant multiplex rate a little
 * above the stream's average rate and a picture's PTS is its index times the picture period; the delivery is not paced
 * against the P-STD / T-STD buffer model (a very large first picture can arrive after its PTS, a long stream runs ahead of
 * the decoder).  Software players and remultiplexers accept that; a hardware or strictly STD-checking demultiplexer needs
 * the stream re-paced by a real multiplexer.
 *
 * MPEG-2 Program Stream (ISO/IEC 13818-1 2.5): packs of at most 2048 bytes, a system header in the first pack, one
 * video PES stream (stream_id 0xE0); every picture starts a PES packet that carries its PTS (no B pictures: DTS =
 * PTS; the sequence headers travel with the first picture), MPEG_program_end_code at the end.  The multiplex
 * rate is derived from the stream size and the frame rate.
 * Call with out = NULL to get the required size in *out_bytes.
 */
int m2vc_mux_ps(const uint8_t *es, size_t es_bytes, uint8_t *out, size_t cap, size_t *out_bytes);

/*
 * MPEG-2 Transport Stream (ISO/IEC 13818-1 2.4): 188-byte packets, PAT (PID 0) + PMT (PID 0x1000) repeated every
 * 0.1 s of stream time, video on PID 0x100 carrying the PCR, one PES packet per picture with PTS.
 * Call with out = NULL to get the required size in *out_bytes.
 */
int m2vc_mux_ts(const uint8_t *es, size_t es_bytes, uint8_t *out, size_t cap, size_t *out_bytes);

/*
 * The inverse: one video elementary stream out of a transport or program stream - ours or an ordinary multiplexer's.  These two
 * serial functions are the definition of what m2v_demux_device (include/m2v_mi355x.h) computes.  They never read outside
 * [src, src + n) whatever the bytes are, and the payload is not assumed to be video: it may hold pack headers, PES headers, start
 * codes and 0x47 at any place.
 *
 * out == NULL asks for the size (info->out_bytes); otherwise the elementary bytes go to out, M2VC_E_OVERFLOW if cap is too small
 * (nothing is written; info->out_bytes = the need).  One m2vc_stamp per PES packet of the stream, in container order: at most
 * stamp_cap are written (stamps may be NULL), info->pes_packets says how many there were.  The return value is info->status:
 *   M2VC_OK
 *   M2VC_E_SYNTAX    info->err_offset = the offset of the EARLIEST packet / unit that breaks a rule below
 *   M2VC_E_NOSTREAM  no PAT / PMT / video entry, or no PES packet of the stream starts anywhere
 *   M2VC_E_OVERFLOW
 * (M2VC_E_PARAM for a NULL src / info or a `stream` out of range: info is not written.)  With a status other than OK every counter
 * of info is 0 (out_bytes too, except for OVERFLOW), and err_offset is 0 unless the status is SYNTAX.
 *
 * Transport stream (188-byte packets; `stream` = the video PID 0 .. 0x1FFF, or -1: found through PAT and PMT).
 *   n must be a positive multiple of 188 (else SYNTAX at 188 * (n / 188)) and byte 0 of every packet 0x47 (SYNTAX at that packet).  A
 *   packet with transport_error_indicator set is ignored whatever its PID.  Discovery: the PAT is the first packet with PID 0,
 *   payload_unit_start_indicator and a payload - pointer_field, then a section with table_id 0, section_syntax_indicator 1, wholly
 *   inside that packet, CRC-32/MPEG 0 (else SYNTAX at the packet); its first entry with program_number != 0 names the PMT PID (none:
 *   NOSTREAM); the PMT is the first such packet of that PID (table_id 2, the same checks, the same program_number); the first entry of
 *   its stream loop with stream_type 1 or 2 names the video PID (none: NOSTREAM), which then holds for every packet of the input.
 *   Discovery does not look at the sync bytes (they have their verdict anyway), and NOSTREAM is answered only where no rule is broken:
 *   a broken rule anywhere is SYNTAX at the earliest one.
 *   Packets of other PIDs are skipped and, beyond the sync byte, not validated.  A video packet: transport_scrambling_control != 0,
 *   adaptation_field_control 0, control 2 with adaptation_field_length != 183 and control 3 with a length > 182 are SYNTAX; of the
 *   adaptation field only discontinuity_indicator is read.  With payload_unit_start_indicator the payload starts with a PES header of
 *   9 + hl bytes inside this packet (SYNTAX otherwise; see below) and the elementary bytes are the rest; without it the whole payload
 *   is elementary bytes - except in front of the first packet with the indicator: those video packets are dropped and counted in
 *   info->skipped (a stream may be joined in mid-packet).  PES_packet_length is not interpreted: a PES packet runs to the next one.
 *   Continuity is looked at among the video packets that carry a payload, in order: a counter that is not the previous one + 1 mod 16
 *   is counted in info->discontinuities unless that packet's discontinuity_indicator is set.  Nothing is dropped for it, and DUPLICATE
 *   PACKETS ARE NOT REMOVED (a repeated packet's payload appears twice, and counts as a discontinuity).  info->packets = the video
 *   packets (the skipped ones included), info->stream = the PID.
 *
 * Program stream: a serial chain from p = 0 (`stream` = the stream_id 0xE0 .. 0xEF, or -1: that of the chain's first video packet).
 *   p == n ends it.  Otherwise src[p .. p+4) must be 00 00 01 c (else SYNTAX at p).  c == B9 ends the chain: every byte behind it must be
 *   zero (SYNTAX at the first that is not).  c == BA: an MPEG-2 pack header of 14 bytes ('01' and the five marker bits, marker bits
 *   '11' behind the rate; an MPEG-1 one is SYNTAX) and pack_stuffing_length 0 .. 7 bytes, all inside n.  c == BB or c >= BC: a unit
 *   with a 16-bit length L at p + 4, p + 6 + L <= n (else SYNTAX at p); a packet of the selected stream has its PES header parsed
 *   (L >= 3, hl <= L - 3), its elementary bytes are src[p + 9 + hl .. p + 6 + L); every other id is skipped by its length (counted in
 *   info->skipped).  Any other c is SYNTAX at p.  No packet of the selected stream in the whole chain: NOSTREAM.  info->packets = the
 *   pack headers, info->stream = the stream_id, info->discontinuities = 0.
 *
 * PES header (both kinds): 00 00 01, stream_id E0 .. EF, '10', PES_scrambling_control 0, hl = PES_header_data_length.
 *   PTS_DTS_flags 2: hl >= 5, prefix '0010' and three marker bits; 3: hl >= 10, prefixes '0011' / '0001'; 0: neither; 1 is SYNTAX.  The
 *   rest of the header is skipped by hl.
 */
#define M2VC_E_NOSTREAM (-4)
typedef struct { uint64_t es_offset, pts, dts, src_offset; } m2vc_stamp;      /* 32 bytes; pts / dts = ~0 when absent; src_offset = the PES header's place */
typedef struct { uint64_t out_bytes, err_offset; uint32_t pes_packets, packets, discontinuities, skipped, stream; int32_t status; } m2vc_demux_info;
int m2vc_demux_ts(const uint8_t *src, size_t n, int stream, uint8_t *out, size_t cap, m2vc_stamp *stamps, size_t stamp_cap,
                  m2vc_demux_info *info);
int m2vc_demux_ps(const uint8_t *src, size_t n, int stream, uint8_t *out, size_t cap, m2vc_stamp *stamps, size_t stamp_cap,
                  m2vc_demux_info *info);

#ifdef __cplusplus
}
#endif
#endif
