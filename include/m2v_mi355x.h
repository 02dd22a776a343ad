/*
 * m2v_mi355x.h — C-ABI of the MI355X-native MPEG-2 I/P encoder (libm2v_mi355x.so).
 *
 * The reference exposes no software API: its interface is the port list of the Verilog module
 * `mpeg2encoder` (RTL/mpeg2encoder.v:10-38) driven by SIM/tb_mpeg2encoder.v.  Each entry point
 * below replaces one part of that port contract and cites it.  Plain pointers and sizes only; no
 * torch / HIP types in the signatures (a stream is passed as an opaque void*).
 *
 * One handle = one encoder instance = one GPU + one HIP stream.  Handles are independent
 * (config "8 sequences on 8 GPUs" = 8 handles); a handle is not re-entrant.  All functions
 * return 0 / a count on success and a negative M2V_E_* code on failure;
 * m2v_last_error() gives the text.  There is NO CPU fallback: without a GPU m2v_create() fails.
 */
#ifndef M2V_MI355X_H
#define M2V_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct m2v_enc m2v_enc;

enum {
    M2V_OK          = 0,
    M2V_E_PARAM     = -1,   /* XL/YL/VECTOR_LEVEL/Q_LEVEL outside the ranges of RTL:11-14          */
    M2V_E_NODEVICE  = -2,   /* no usable HIP device                                                 */
    M2V_E_HIP       = -3,   /* a HIP call failed                                                    */
    M2V_E_STATE     = -4,   /* call not legal in the current sequence state                         */
    M2V_E_NOMEM     = -5,
    M2V_E_OVERFLOW  = -6    /* caller-provided output buffer too small                              */
};

/* Library version / build string (for logs). */
const char *m2v_version(void);

/*
 * Module instantiation: `mpeg2encoder #(XL, YL, VECTOR_LEVEL, Q_LEVEL)` (RTL:10-15) plus the one
 * required reset (RTL:16, README "rstn").  XL,YL in 4..7 (max 16<<XL x 16<<YL pixels),
 * VECTOR_LEVEL in 1..3, Q_LEVEL in 1..4.  `device` = HIP device ordinal.
 * Returns NULL on failure; *err (optional) receives the M2V_E_* code.
 */
m2v_enc *m2v_create(int XL, int YL, int VECTOR_LEVEL, int Q_LEVEL, int device, int *err);
void     m2v_destroy(m2v_enc *e);

/* PCI address ("0000:c1:00.0") of HIP device `device`, NUL-terminated into buf: which card of /sys/class/drm a handle created on that
 * ordinal runs on (sensors, topology).  Returns the string's length, M2V_E_NODEVICE for an ordinal out of range, M2V_E_PARAM for a
 * buffer of less than 16 bytes.  No counterpart in the RTL: a host-side aid. */
int m2v_device_pci_bus_id(int device, char *buf, size_t cap);

/* `rstn` low (RTL:1028-1039): drop any sequence in flight, return to idle, discard output. */
int m2v_reset(m2v_enc *e);

/*
 * Pixel input: `i_en` + i_Y0..3 / i_U0..3 / i_V0..3, 4 horizontally adjacent 4:4:4 pixels per
 * beat, raster order, frame after frame (RTL:25-28, README:98-197).  y4/u4/v4 hold nbeats*4
 * bytes each.  i_xsize16 / i_ysize16 / i_pframes_count (RTL:20-22) are sampled on the first beat
 * of a sequence only (RTL:1060-1065) and ignored afterwards; out-of-range sizes follow the RTL
 * clamp (RTL:985-991).  `stop_with_last` != 0 raises i_sequence_stop together with the last
 * beat (RTL:1082-1083).  Beats arriving while the previous sequence is still ending are dropped
 * like the RTL does (RTL:1045-1058) — pull the output until `last` first.
 */
int m2v_push_beats(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                   const uint8_t *y4, const uint8_t *u4, const uint8_t *v4, size_t nbeats,
                   int stop_with_last);

/*
 * The same beats from a packed 4:4:4 source: `pixels` holds nbeats*4 pixels in raster order, each pixel
 * `layout` bytes wide (the twelve port bytes i_Y0..3/i_U0..3/i_V0..3 of RTL:25-28, interleaved the way
 * capture hardware delivers them).  Everything else as m2v_push_beats.
 */
enum {
    M2V_PACKED_YUV24  = 0,   /* Y U V            3 bytes per pixel */
    M2V_PACKED_UYV24  = 1,   /* U Y V            3 bytes per pixel */
    M2V_PACKED_YUVX32 = 2,   /* Y U V x          4 bytes per pixel, 4th ignored */
    M2V_PACKED_AYUV32 = 3    /* A Y U V          4 bytes per pixel, 1st ignored */
};
int m2v_push_packed(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                    const uint8_t *pixels, size_t nbeats, int layout, int stop_with_last);

/*
 * Convenience = nframes * W*H/4 beats from planar frames laid out like the testbench's files
 * (Y plane, U plane, V plane per frame, each W*H bytes; SIM/tb_mpeg2encoder.v:210-234).
 * W,H are the CLAMPED sizes (m2v_geometry).
 */
int m2v_push_frames(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                    const uint8_t *frames444, size_t nframes);

/*
 * Whole 4:2:0 frames, as decoders, cameras and ordinary .yuv files deliver them.  The module has no 4:2:0 port; the first thing it does
 * with its 4:4:4 samples is the two-stage mean2 down-conversion (RTL:1086-1089, 1167-1170), and mean2(a, a) = a.  So by definition the
 * stream of a 4:2:0 frame is, byte for byte, the stream of the 4:4:4 frame whose U and V planes are the 4:2:0 planes with every sample
 * repeated 2 x 2: the encoder codes the caller's chroma, unfiltered.  W, H are the CLAMPED sizes (m2v_geometry), multiples of 16; a
 * frame is W*H*3/2 bytes in one of these layouts:
 */
enum {
    M2V_420_I420 = 0,        /* Y (W*H), U (W*H/4), V (W*H/4)                      */
    M2V_420_YV12 = 1,        /* Y, V, U                                            */
    M2V_420_NV12 = 2,        /* Y, then H/2 rows of W bytes U V U V ...            */
    M2V_420_NV21 = 3         /* Y, then H/2 rows of W bytes V U V U ...            */
};
/*
 * m2v_push_frames for `nframes` such frames, with every promise of it: the sizes and pframes_count are sampled on the first frame of a
 * sequence only, frames are dropped while the previous sequence is ending, M2V_E_STATE while a frame is partly filled by m2v_push_beats,
 * page-locked sources cross the link from where they are (option "direct_upload", 2 and m2v_upload_wait included), anything else goes
 * through the pinned staging.  Half the bytes of the 4:4:4 form cross the link; the frames are expanded on the device in front of
 * the chunk's kernels.  4:4:4 frames, packed beats and 4:2:0 frames may alternate inside one sequence.  M2V_E_PARAM for an unknown
 * layout.  There are no 4:2:0 beats: half a chroma row has no meaning at the port.
 */
int m2v_push_frames420(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                       const uint8_t *frames420, size_t nframes, int layout);

/*
 * Whole RGB frames, as renderers, screen grabbers and image tensors hold them.  The module has no RGB port, so the behaviour is a
 * definition: the stream of an RGB frame is, byte for byte, the stream of the planar 4:4:4 frame obtained by the integer transform
 * below; the module's own two-stage mean2 then makes the 4:2:0 chroma from those planes as for any 4:4:4 caller.  Per pixel, with
 * (R, G, B) in 0 ... 255, a matrix T of 3 x 3 integers (scale 2^14) and a luma offset o (>> is arithmetic, i.e. floor):
 *
 *     Y = clamp(((T00*R + T01*G + T02*B + 8192) >> 14) + o,   0, 255)
 *     U = clamp(((T10*R + T11*G + T12*B + 8192) >> 14) + 128, 0, 255)        U = Cb
 *     V = clamp(((T20*R + T21*G + T22*B + 8192) >> 14) + 128, 0, 255)        V = Cr
 *
 *     matrix           T (rows Y, U, V; columns R, G, B)                                   o
 *     M2V_RGB_BT601    4207  8260 1604 / -2428 -4768 7196 / 7196 -6026 -1170              16    studio range, 16-235 / 16-240
 *     M2V_RGB_BT709    2991 10064 1016 / -1649 -5547 7196 / 7196 -6536  -660              16    studio range
 *     M2V_RGB_BT601F   4899  9617 1868 / -2765 -5427 8192 / 8192 -6860 -1332               0    full range (JFIF)
 *     M2V_RGB_BT709F   3483 11718 1183 / -1877 -6315 8192 / 8192 -7441  -751               0    full range
 *
 * With Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709), sy, sc = 219/255, 224/255 (studio) or 1, 1 (full) and
 * r(x) = floor(x * 2^14 + 1/2):  T00 = r(Kr*sy), T02 = r(Kb*sy), T01 = r(sy) - T00 - T02;  T12 = r(sc/2), T10 = r(-Kr*sc / (2(1-Kb))),
 * T11 = -T10 - T12;  T20 = r(sc/2), T22 = r(-Kb*sc / (2(1-Kr))), T21 = -T20 - T22.  The middle coefficient is the remainder on
 * purpose: every grey gives exactly 128 / 128 and white exactly 235 (or 255).  The result is within 0.508 of the real-valued
 * transform for every input; the clamp only ever acts in the two full-range matrices (Cb / Cr of pure blue / pure red reach 256).
 *
 * The stream DOES carry a colour description: the module writes a sequence_display_extension (RTL:2612-2617) whose colour_primaries /
 * transfer_characteristics / matrix_coefficients are 5 / 5 / 5 (BT.470BG, BT.601), whatever matrix made the samples.  The conversion
 * does not change it - the stream stays what the module would emit for those samples -, so a caller that converts with M2V_RGB_BT709
 * says so itself: m2v_set_stream_desc with 1 / 1 / 1.
 */
enum {
    M2V_RGB_BT601 = 0,
    M2V_RGB_BT709 = 1,
    M2V_RGB_BT601F = 2,
    M2V_RGB_BT709F = 3
};
/* Layouts: a frame is W*H*bpp bytes in raster order, W, H the CLAMPED sizes (m2v_geometry). */
enum {
    M2V_RGB_RGB24 = 0,       /* R G B, 3 bytes per pixel                                            */
    M2V_RGB_BGR24 = 1,       /* B G R                                                               */
    M2V_RGB_RGBX32 = 2,      /* R G B x, 4 bytes per pixel, the 4th ignored (RGBA)                  */
    M2V_RGB_BGRX32 = 3,      /* B G R x (BGRA)                                                      */
    M2V_RGB_XRGB32 = 4,      /* x R G B (ARGB)                                                      */
    M2V_RGB_XBGR32 = 5,      /* x B G R (ABGR)                                                      */
    M2V_RGB_RGBP = 6         /* planar: R plane, G plane, B plane, W*H bytes each (a [3, H, W] image) */
};
/* The table above, readable without a GPU: coeff[9] row by row, *y_offset = o.  M2V_E_PARAM for an unknown matrix. */
int m2v_rgb_matrix(int matrix, int coeff[9], int *y_offset);
/*
 * m2v_push_frames420 for `nframes` RGB frames, with every promise of it: parameters sampled on the first frame of a sequence only,
 * frames dropped while the previous sequence is ending, M2V_E_STATE while a frame is partly filled by m2v_push_beats, page-locked
 * sources cross the link from where they are (option "direct_upload", 2 and m2v_upload_wait included), anything else goes through the
 * pinned staging.  The frames are converted on the device in front of the chunk's kernels.  RGB frames may alternate with 4:4:4
 * frames, packed beats and 4:2:0 frames inside one sequence, and with RGB frames of another layout or matrix.  M2V_E_PARAM for an
 * unknown layout or matrix.  Whole frames only: there are no RGB beats.
 */
int m2v_push_rgb(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                 const uint8_t *frames, size_t nframes, int layout, int matrix);

/*
 * Frames of any size.  The module takes whole macroblocks only, and its README tells the user to pad ("a 1910x1080 video should be
 * padded to 1920x1088").  With a size set, every whole-frame entry - m2v_push_frames, m2v_push_frames420, m2v_push_rgb and their _pull
 * forms, m2v_encode_resident, m2v_encode_resident420, m2v_encode_resident_rgb and their _begin forms - takes frames of width x height
 * pixels in its own format and pads them on the device (k_fit) in front of what it did before; only the source's bytes cross the link.
 *
 * DEFINITION.  W = 16 * ceil(width / 16), H = 16 * ceil(height / 16).  The padded frame has the format of the source; every plane is
 * extended to the right and then downwards by repeating its last column and its last row (numpy.pad(..., mode = "edge")):
 *
 *     planar 4:4:4        Y, U, V: 1 byte, width x height                                     -> W x H
 *     I420 / YV12         Y: 1 byte, width x height; two chroma planes: 1 byte, cw x ch       -> W x H; W/2 x H/2
 *     NV12 / NV21         Y: 1 byte, width x height; one plane of 2-byte pairs, cw x ch       -> W x H; W/2 x H/2
 *     RGB24 / BGR24       one plane of 3-byte pixels, width x height                          -> W x H
 *     RGBX32 ... XBGR32   one plane of 4-byte pixels (the ignored byte travels with its pixel)   -> W x H
 *     RGBP                R, G, B: 1 byte, width x height                                     -> W x H
 *
 * cw = (width + 1) / 2, ch = (height + 1) / 2 (integer division; odd sizes are legal), so a 4:2:0 source frame is
 * width * height + 2 * cw * ch bytes.  4:2:0 chroma is padded in the 4:2:0 domain, before the 2 x 2 repeat.  Frames lie back to back
 * with no alignment between them; only the base pointer of a resident 4:2:0 or RGB call keeps its 16-byte rule.  The stream is byte
 * for byte the stream of those padded frames at xsize16 = W / 16, ysize16 = H / 16, and the call that starts a sequence must pass
 * exactly these (m2v_fit_size): anything else is M2V_E_PARAM with nothing started.
 *
 * header: what sequence_header (12 + 12 bits, stream bytes 4 - 6) and sequence_display_extension (14 + 1 + 14 bits from byte 30) say.
 *     M2V_HEADER_MODULE   W x H, as the module fed the padded frames writes it: a player shows the padding
 *     M2V_HEADER_TRUE     width x height in those four fields and no other bit of the stream differs.  NOT the module's behaviour
 *                         (like option "conformant"): ISO/IEC 13818-2 defines the fields as the displayable size and derives the
 *                         macroblock count by rounding up, so this is the conformant stream of, say, a 1080-line picture.
 *     Caveat, documented and not acted on: the module sets progressive_sequence = 0, and under that setting ISO derives the macroblock
 *     rows as 2 * ceil(height / 32).  That equals the coded ceil(height / 16) rows only where the latter is even (1080 -> 68: yes).
 *     The same already holds for the module's own streams with an odd number of macroblock rows.
 *
 * Only while the handle is idle (M2V_E_STATE otherwise); the setting stays until it is changed, m2v_reset keeps it, (0, 0, x) switches
 * it off.  M2V_E_PARAM for a negative size, for one size zero and the other not, for a padded size outside 64 ... 16 << XL by
 * 64 ... 16 << YL (so width, height >= 49), and for an unknown header.  A size of whole macroblocks launches no padding pass and
 * behaves as no size set.  While a size is set m2v_push_beats, m2v_push_packed and every m2v_strip_* entry that starts something answer
 * M2V_E_STATE: the port has no partial macroblock, and strips take whole padded frames.
 */
enum { M2V_HEADER_MODULE = 0, M2V_HEADER_TRUE = 1 };
int m2v_set_frame_size(m2v_enc *e, int width, int height, int header);
/* xsize16 = ceil(width / 16), ysize16 = ceil(height / 16): pure arithmetic, no GPU.  M2V_E_PARAM for a size below 1. */
int m2v_fit_size(int width, int height, uint32_t *xsize16, uint32_t *ysize16);

/*
 * Frames of another size, resampled on the device.  The module's README tells its users to pad and says nothing about a source of
 * another size, so - as with 4:2:0, RGB and padding - the behaviour is a definition of ours.  While a source size is set, every
 * resident whole-frame entry - m2v_encode_resident, m2v_encode_resident420, m2v_encode_resident_rgb and their _begin forms - takes
 * frames of src_width x src_height pixels in its own format and resamples them on the device (k_scale) in front of what it did before.
 *
 * DEFINITION.  The picture size w x h is the size set with m2v_set_frame_size, or W x H of the starting call's xsize16, ysize16 when
 * none is set.  The stream is byte for byte the stream the same entry gives for the frames pad(scale(x)): every plane of the source
 * frame is resampled to the picture size in the source's own format, the result is padded to whole macroblocks as m2v_set_frame_size
 * defines, and that is converted as before.  Planes and elements are those of the table above, with sw x sh for width x height:
 *
 *     planar 4:4:4, RGBP  three planes of sw x sh bytes                                  -> w x h
 *     I420 / YV12         Y: sw x sh; two chroma planes of scw x sch                     -> w x h; cw x ch
 *     NV12 / NV21         Y: sw x sh; one plane of 2-byte pairs, scw x sch               -> w x h; cw x ch
 *     RGB24 / BGR24       one plane of 3-byte pixels, sw x sh                            -> w x h
 *     RGBX32 ... XBGR32   one plane of 4-byte pixels, sw x sh                            -> w x h
 *
 * scw = (sw + 1) / 2, sch = (sh + 1) / 2, cw = (w + 1) / 2, ch = (h + 1) / 2.  Every byte of an element is filtered on its own with its
 * plane's taps; the ignored byte of a 32-bit pixel may hold anything afterwards, nothing reads it.  4:2:0 chroma is resampled in the
 * 4:2:0 domain, plane by plane, centre-aligned like luma: CHROMA SITING IS NOT MODELLED (a left-sited source keeps its samples a
 * fraction of a chroma sample from where MPEG-2 expects them, as every centre-aligned scaler leaves them).  A source frame is
 * sw * sh + 2 * scw * sch bytes (4:2:0), sw * sh * 3 or sw * sh * 4; frames lie back to back at any address, only the base pointer of
 * a resident 4:2:0 or RGB call keeps its 16-byte rule.
 *
 * Taps of one dimension, src samples to dst samples, output index x, all in integers, sample centres aligned:
 *
 *     M2V_SCALE_TRIANGLE  P = (2x + 1) * src - dst, R = 2 * max(src, dst), a(i) = R - |2 * dst * i - P| over every integer i with
 *                         a(i) > 0 (i may lie below 0 or above src - 1): bilinear when enlarging, a triangle widened by the ratio
 *                         when reducing
 *     M2V_SCALE_AREA      a(i) = min((i + 1) * dst, (x + 1) * src) - max(i * dst, x * src) over every i with a(i) > 0: the exact area
 *                         of source sample i under output sample x
 *
 * With first the smallest such i, n their count (they are contiguous) and A their sum: c(i) = floor(a(i) * 2^14 / A), and the remainder
 * 2^14 - sum c(i) goes onto the tap with the largest a(i), the lowest i among equals.  A tap reads sample clamp(i, 0, src - 1): weight
 * that falls outside the plane lands on its edge sample.  The horizontal pass comes first, on every source row r,
 *
 *     t[r][x] = (sum c_x(i) * s[r][clamp i] + 128) >> 8                 (0 ... 16320)
 *
 * and the vertical pass follows, with the taps d_y(j) of the other dimension:
 *
 *     o[y][x] = (sum d_y(j) * t[clamp j][x] + 2^19) >> 20
 *
 * There is no clamp of the result: the coefficients are not negative and sum to 2^14.  Equal sizes give the single tap (x, 2^14): the
 * identity.  Every output lies within 1.45 of the same taps in real arithmetic (255 * 2 * 15 / 2^14 = 0.467 of coefficient error per
 * pass, 1 / 128 of the first rounding, 0.5 of the second).
 *
 * Limits: 1 <= src_width, src_height <= 16384, and src_width <= 8 * w, src_height <= 8 * h (the chroma planes then stay within 8 as
 * well), which bounds a tap list at M2V_SCALE_MAXTAPS; enlarging has no limit.  The call that starts a sequence checks the ratio
 * against the picture size it now knows: M2V_E_PARAM with nothing started, the text names both sizes.
 *
 * Only while the handle is idle (M2V_E_STATE otherwise); the setting stays until it is changed, m2v_reset keeps it, (0, 0, x) switches
 * it off.  M2V_E_PARAM for a negative size, for one size zero and the other not, for a size above 16384, and for an unknown filter.  A
 * source size equal to the picture size launches no resampling pass and behaves as none set.  m2v_set_frame_size's header modes work
 * as before: the picture size is theirs.  While a source size is set, m2v_push_frames / 420 / rgb and their _pull forms, m2v_push_beats,
 * m2v_push_packed and every m2v_strip_* entry that starts something answer M2V_E_STATE: the port's staging is sized for frames of the
 * coded size, and strips take whole padded frames.
 */
enum { M2V_SCALE_TRIANGLE = 0, M2V_SCALE_AREA = 1 };
#define M2V_SCALE_MAXTAPS 16
int m2v_set_source_size(m2v_enc *e, int src_width, int src_height, int filter);
/* The taps of output sample x (0 ... dst - 1) by the definition above: returns n, *first = the first tap's sample index (may be negative),
 * coeff[0 ... n - 1] = c(first) ..., the rest 0.  Pure arithmetic, no GPU; the single source of the tables the kernel reads.
 * M2V_E_PARAM for an unknown filter, src or dst outside 1 ... 16384, src > 8 * dst, x outside the output.  first and coeff may be NULL. */
int m2v_scale_taps(int filter, int src, int dst, int x, int *first, uint16_t coeff[M2V_SCALE_MAXTAPS]);

/* `i_sequence_stop` pulse with i_en = 0 (RTL:1090-1091; SIM/tb_mpeg2encoder.v:249-252). A frame
 * in progress is completed with black pixels (RTL:1048-1056). No effect while idle. */
int m2v_sequence_stop(m2v_enc *e);
/* Option "direct_upload" = 2 only (a no-op otherwise): waits until every frame handed to m2v_push_frames so far has been read. */
int m2v_upload_wait(m2v_enc *e);

/* `o_sequence_busy` (RTL:1095): 1 from the first beat until the `last` word has been pulled. */
int m2v_busy(const m2v_enc *e);

/*
 * Stream output: `o_en` / `o_data[255:0]` / `o_last` (RTL:35-37, 2961-2994).  Copies up to
 * cap/32 whole 32-byte words, byte 0 = o_data[7:0], in stream order; returns the byte count.
 * *last (optional) is set to 1 when the returned data ends with the o_last word; the encoder is
 * idle again after that.  GPU work is batched in chunks of "batch_frames" frames and runs asynchronously:
 * before the stop, m2v_pull returns the words of the chunks that are complete (possibly none) without
 * waiting; after the stop it waits for the rest.
 */
long long m2v_pull(m2v_enc *e, uint8_t *dst, size_t cap, int *last);
/*
 * Both port groups in ONE call, as the module drives them in the same clock (input beats RTL:15-21 while o_en / o_data run,
 * RTL:35-37; the testbench's producer and consumer blocks, SIM/tb_mpeg2encoder.v:206-266 and :268-281): m2v_push_frames followed by
 * m2v_pull into dst, with the same results and return value as that pair - except that the words of completed chunks are
 * copied into dst WHILE this call's frames cross the link, not between two transfers.  For a caller with one thread and frames in
 * page-locked memory the link then only idles for the caller's own turn-around.
 * On an error (negative return) nothing that was encoded is lost: words that had already been copied into dst inside the failed call are
 * put back at the front of the output FIFO and come out of the next m2v_pull; the contents of dst are then undefined.  After a device
 * error the handle is good for m2v_pull, m2v_reset and m2v_destroy only.
 */
long long m2v_push_frames_pull(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                               const uint8_t *frames444, size_t nframes, uint8_t *dst, size_t cap, int *last);

/* m2v_push_frames_pull for 4:2:0 frames (m2v_push_frames420 followed by m2v_pull into dst, in one call). */
long long m2v_push_frames420_pull(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                                  const uint8_t *frames420, size_t nframes, int layout, uint8_t *dst, size_t cap, int *last);

/* m2v_push_frames_pull for RGB frames (m2v_push_rgb followed by m2v_pull into dst, in one call). */
long long m2v_push_rgb_pull(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                            const uint8_t *frames, size_t nframes, int layout, int matrix, uint8_t *dst, size_t cap, int *last);

/* Clamped geometry the module would use for (xsize16, ysize16) (RTL:985-1006). */
int m2v_geometry(const m2v_enc *e, uint32_t xsize16, uint32_t ysize16, int *width, int *height);

/*
 * Whole-sequence entry for inputs and outputs resident in HBM (what bench.py times): encodes
 * `nframes` planar 4:4:4 frames at device pointer `d_frames444` as ONE sequence (first beat ..
 * stop after the last beat) and leaves the stream at `d_out` (capacity cap bytes, 4-byte aligned).
 * The byte count goes to *out_bytes after the work completes; `hip_stream` (a hipStream_t or NULL
 * for the handle's own stream) is synchronised before returning.  The encoder must be idle.
 */
int m2v_encode_resident(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                        const void *d_frames444, size_t nframes, void *d_out, size_t cap,
                        size_t *out_bytes, void *hip_stream);
/*
 * The same in two halves, for callers that keep more than one sequence in flight (several handles, each with its own work
 * buffers and streams: the stream assembly of one sequence then runs beside the first macroblock kernels of the next instead of
 * leaving the GPU to drain).  _begin enqueues the whole sequence on `hip_stream` and returns without waiting; _end waits for that
 * stream and hands out the byte count.  Between the two the handle accepts no other call but m2v_reset / m2v_destroy (both wait
 * for the sequence first, on whichever stream it was given; everything else answers M2V_E_STATE), and the input and output buffers
 * belong to the encoder.  (A sequence longer than "batch_frames" is still encoded chunk by chunk, with a
 * wait between the chunks inside _begin.)
 */
int m2v_encode_resident_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                              const void *d_frames444, size_t nframes, void *d_out, size_t cap, void *hip_stream);
int m2v_encode_resident_end(m2v_enc *e, size_t *out_bytes);
/*
 * The resident entries for 4:2:0 frames (M2V_420_*, W*H*3/2 bytes each, back to back at the 16-byte aligned device pointer
 * `d_frames420`): each chunk is expanded into a planar 4:4:4 buffer the handle owns, on the call's stream in front of the chunk's
 * kernels.  Everything else as m2v_encode_resident / m2v_encode_resident_begin; the latter is answered by m2v_encode_resident_end.
 */
int m2v_encode_resident420(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                           const void *d_frames420, size_t nframes, int layout, void *d_out, size_t cap,
                           size_t *out_bytes, void *hip_stream);
int m2v_encode_resident420_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                                 const void *d_frames420, size_t nframes, int layout, void *d_out, size_t cap, void *hip_stream);
/*
 * The resident entries for RGB frames (M2V_RGB_* layout and matrix, W*H*bpp bytes each, back to back at the 16-byte aligned device
 * pointer `d_frames`): each chunk is converted into the planar 4:4:4 buffer the handle owns, on the call's stream in front of the
 * chunk's kernels.  Everything else as m2v_encode_resident / m2v_encode_resident_begin; the latter is answered by
 * m2v_encode_resident_end.
 */
int m2v_encode_resident_rgb(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                            const void *d_frames, size_t nframes, int layout, int matrix, void *d_out, size_t cap,
                            size_t *out_bytes, void *hip_stream);
int m2v_encode_resident_rgb_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                                  const void *d_frames, size_t nframes, int layout, int matrix, void *d_out, size_t cap,
                                  void *hip_stream);

/*
 * Strip mode (BASELINE config c5; no RTL counterpart — the RTL has one reference BRAM): several
 * handles, one per GPU, each encode the macroblock rows [row0,row1) of EVERY frame of one sequence.
 * Slices are byte-aligned and reset all predictors (RTL:2704-2715), so strips only interact through
 * the +-2*VECTOR_LEVEL luma / +-VECTOR_LEVEL chroma rows of the previous reconstruction next to
 * the strip boundary (window geometry RTL:1446-1448).  The caller moves those rows between GPUs
 * (RCCL send/recv over xGMI in fpga-mpeg2-encoder_amd/parallel.py) between the steps:
 *
 *   m2v_strip_begin(...)                         plan the whole sequence as one chunk
 *   m2v_strip_info(&steps, &halo_bytes)          steps = frames per GOP in the chunk
 *   for j in 0..steps-1:
 *       n = m2v_strip_step(j, send_up, send_down) (or _edges / _interior around the exchange, see below)
 *                                                macroblock kernel for the j-th frame of every GOP, then
 *                                                packs this strip's top / bottom rows of the n frames that are
 *                                                referenced later: n * 3*VECTOR_LEVEL*W bytes per direction
 *       <exchange: send_up -> rank-1's from_down, send_down -> rank+1's from_up>
 *       m2v_strip_halo_in(j, from_up, from_down) neighbour rows into the reconstruction buffers
 *   m2v_strip_finish(d_strip, cap, frame_off)    this strip's slices of every frame, contiguous;
 *                                                frame_off[f]..frame_off[f+1] = bytes of frame f (nframes+1 entries)
 *   m2v_strip_assemble(...)                      on the rank that owns the output: headers + strips
 *                                                of all ranks -> the final stream (enqueued, NOT synchronised:
 *                                                *out_bytes is valid at return, the bytes in stream order)
 * Everything is enqueued on the stream given to m2v_strip_begin (NULL = the handle's own stream).
 * Buffers are device pointers except frame_off (host).
 * Alignment (m2v_strip_assemble and the output rank of m2v_strip_encode move the strips with 16-byte stores and read them as
 * aligned dwords): d_out 16-byte aligned, every d_strips[r] 4-byte aligned with a capacity that is a multiple of 4 (the dword
 * that holds a strip's last byte is read whole); M2V_E_PARAM otherwise.  hipMalloc'ed buffers satisfy both.
 */
int m2v_strip_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                    const void *d_frames444, size_t nframes, int row0, int row1, void *hip_stream);
int m2v_strip_info(const m2v_enc *e, int *steps, size_t *halo_bytes_per_direction);
int m2v_strip_step(m2v_enc *e, int step, void *d_send_up, void *d_send_down);
/* The same step in two parts, so that the exchange overlaps with compute: _edges encodes the first
 * and the last macroblock row of the strip and packs their halo (same return value as m2v_strip_step); the caller
 * starts the send/recv; _interior encodes the rows in between while the halo is in flight; then m2v_strip_halo_in. */
int m2v_strip_step_edges(m2v_enc *e, int step, void *d_send_up, void *d_send_down);
int m2v_strip_step_interior(m2v_enc *e, int step);
int m2v_strip_halo_in(m2v_enc *e, int step, const void *d_from_up, const void *d_from_down);
int m2v_strip_finish(m2v_enc *e, void *d_strip, size_t cap, unsigned long long *frame_off);
/* The same in two halves: _async enqueues the scans and the slice assembly and returns at once; m2v_strip_offsets waits for
 * them (one event, pinned read-back) and hands out the nframes + 1 offsets.  m2v_strip_finish = both. */
int m2v_strip_finish_async(m2v_enc *e, void *d_strip, size_t cap);
int m2v_strip_offsets(m2v_enc *e, unsigned long long *frame_off);
int m2v_strip_assemble(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count,
                       size_t nframes, int nranks, const void *const *d_strips,
                       const unsigned long long *const *frame_off, void *d_out, size_t cap,
                       size_t *out_bytes, void *hip_stream);

/*
 * The exchange between the strips, behind one opaque communicator (csrc/m2v_comm.hpp).  Two kinds:
 *   RCCL    one process per GPU (ncclGroupStart; ncclSend / ncclRecv x 2; ncclGroupEnd per GOP step over xGMI, one
 *           ncclAllGather of the strip sizes and one group of sends into the output rank per sequence).  librccl is dlopen()ed
 *           on first use.  Rank 0 calls m2v_comm_unique_id (128 bytes), the caller broadcasts them by whatever means it has
 *           (torch.distributed, MPI, a file), every rank calls m2v_comm_init_rccl - a collective call, like ncclCommInitRank.
 *   local   `world` handles inside ONE process, one host thread each (on one GPU or several): mailboxes of device pointers and
 *           events, device-to-device copies.  One object shared by all the threads.  Runs the N-rank path on a 1-GPU box.
 * m2v_comm_last_error(): why the last m2v_comm_* call on this thread failed.
 */
typedef struct m2v_comm m2v_comm;
int       m2v_comm_unique_id(void *id, size_t cap);      /* returns 128, or a negative M2V_E_* (no librccl) */
m2v_comm *m2v_comm_init_rccl(const void *id, int rank, int world, int device, int *err);
m2v_comm *m2v_comm_init_local(int world, int *err);
/* Timing aid, NOT an encoder: one rank of `world` alone on its GPU; the halo it "receives" is its own rows, the sizes are its own,
 * nothing is sent.  The resulting stream is not a valid encoding; tools/strip_solo.py uses it to time what one rank of an
 * N-GPU job does per GOP step when only one GPU is at hand. */
m2v_comm *m2v_comm_init_solo(int world, int *err);
/* The same with the rows travelling through a 1-rank RCCL communicator: ncclGroupStart; ncclSend / ncclRecv addressed to the rank
 * itself; ncclGroupEnd - RCCL's call pattern and RCCL's kernels on the stream, with one GPU. */
m2v_comm *m2v_comm_init_solo_rccl(int world, int *err);
void      m2v_comm_destroy(m2v_comm *c);
const char *m2v_comm_last_error(void);
/* Self-test of a communicator: nbytes from d_send to d_recv (device memory) through the transport's own send / recv pair
 * addressed to the calling rank itself (RCCL: one ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd), enqueued on hip_stream. */
int       m2v_comm_selftest(m2v_comm *c, int rank, const void *d_send, void *d_recv, size_t nbytes, void *hip_stream);
/* The same pair once directly, then recorded into a hipGraph (stream capture) and launched `launches` times; the stream is
 * synchronised before returning.  M2V_E_STATE for a communicator that cannot be recorded (the in-process one blocks on other
 * threads).  This is the check that a transport can take part in the recorded sequence of m2v_strip_encode. */
int       m2v_comm_selftest_captured(m2v_comm *c, int rank, const void *d_send, void *d_recv, size_t nbytes, void *hip_stream, int launches);

/*
 * The exchange supplied by the CALLER: three functions of the host program (its MPI, its torch.distributed process group, a test's
 * pipes) behind the communicator interface.  Every pointer is DEVICE memory; `hip_stream` is the stream the data is ordered on, and
 * the function must leave its effect ordered on that stream (enqueue there - or synchronise it, move the bytes, and return).
 * Return 0 for success; anything else fails the m2v_strip_encode call with M2V_E_HIP.
 *   halo           nbytes to / from the rank above (rank - 1) and the rank below (rank + 1); a null pair = no neighbour on that side
 *   allgather_u64  every rank's `count` values into d_all[world][count] on every rank
 *   gather         rank != dst sends sizes[rank] bytes of d_strip to dst, which receives sizes[r] bytes of rank r in bufs[r]
 */
typedef struct m2v_comm_callbacks {
    int (*halo)(void *user, int rank, const void *d_send_up, void *d_recv_up, const void *d_send_down, void *d_recv_down, size_t nbytes, void *hip_stream);
    int (*allgather_u64)(void *user, int rank, const unsigned long long *d_src, unsigned long long *d_all, size_t count, void *hip_stream);
    int (*gather)(void *user, int rank, int dst, const void *d_strip, const size_t *sizes, void *const *bufs, void *hip_stream);
    void *user;
} m2v_comm_callbacks;
m2v_comm *m2v_comm_init_callbacks(int world, const m2v_comm_callbacks *cb, int *err);

/*
 * The PEER transport ("or peer-to-peer stores over xGMI"): a communicator on top of another one (`base`: RCCL, local,
 * callbacks, solo - not owned, destroy this one first) that takes the halo exchange OUT of the GOP step.  Every rank owns a landing
 * block in fine-grained device memory; its neighbours map it (the same process: the pointer + hipDeviceEnablePeerAccess across GPUs;
 * another process: hipIpcOpenMemHandle); the macroblock kernel of the strip's edge rows stores their outer 2 VECTOR_LEVEL luma /
 * VECTOR_LEVEL chroma rows of the reconstruction (RTL:1446-1448) straight into the neighbour's block with write-through stores and
 * counts its arrival there; the next step's edge blocks wait - bounded - for the neighbours' count before they load their window.
 * A GOP step is then ONE launch (edge rows first in dispatch order), no exchange kernel, no second stream.  Sizes and strips still go
 * through `base`.  A wait that runs out of budget (M2V_PEER_BUDGET_US, default 200 000) is not an error: every rank sees it in the
 * all-gathered sizes, the sequence is encoded again exchanging through `base`, and the communicator stays with `base` from then on
 * (m2v_comm_peer_stats says so) - which is what happens when several ranks share ONE GPU and the waiting blocks of one keep the
 * blocks of another from being scheduled.  m2v_strip_encode uses the peer form for the usual form of the step (not with options
 * conformant / dct_mfma = 0) when a step's rows fit `halo_bytes` per direction ((frames of the step) x 9 VECTOR_LEVEL/3 x width).
 *   m2v_comm_init_peer     allocates the block (halo_bytes = 0: 4 MiB per buffer)
 *   m2v_comm_peer_export   this rank's descriptor (M2V_PEER_DESC_BYTES of plain bytes: process, device, address, IPC handle)
 *   m2v_comm_peer_connect  the neighbours' descriptors (NULL where the rank has no neighbour)
 *   m2v_comm_peer_connect_all = export + all-gather through `base` + connect: collective over `base` (solo bases: the rank connects
 *                          to itself, the timing aid's "its own rows come back")
 * Status: byte-identical on one GPU (ranks = threads, and ranks = processes through IPC handles); never run between two GPUs - RCCL
 * stays what bench.py uses by default for N > 1.
 */
#define M2V_PEER_DESC_BYTES 128
m2v_comm *m2v_comm_init_peer(m2v_comm *base, int rank, int device, size_t halo_bytes, int *err);
int       m2v_comm_peer_export(m2v_comm *c, void *desc, size_t cap);
int       m2v_comm_peer_connect(m2v_comm *c, const void *desc_up, const void *desc_down);
int       m2v_comm_peer_connect_all(m2v_comm *c);
/* sequences that ran in the peer form, waits that gave up; returns 1 if the communicator has fallen back to its base for good, 0 if not,
 * M2V_E_PARAM for a communicator without the peer transport */
int       m2v_comm_peer_stats(m2v_comm *c, unsigned long long *peer_sequences, unsigned long long *giveups);
/* what kind of communicator this is: "rccl", "local", "solo", "solo-rccl", "callbacks", "peer+<base>" */
const char *m2v_comm_kind(const m2v_comm *c);

/*
 * One strip of one sequence, start to finish, in ONE call: the loop that parallel.encode_strips() spells out in Python (begin,
 * per GOP step edge rows -> exchange beside the interior rows -> neighbour rows in, finish, sizes, strips to `dst_rank`, final
 * assembly there), natively and without an interpreter between the steps.  Rank r of `world` encodes macroblock rows
 * [r * mbh / world ...) - the partition of parallel.partition_rows().  `comm` may be NULL iff world == 1.  On dst_rank the
 * stream is left at d_out (device memory, capacity cap) and its length in *out_bytes; the other ranks may pass NULL / 0 and
 * get *out_bytes = 0.  `hip_stream` (NULL = the handle's own) is synchronised before returning.  Collective: every rank
 * of the communicator must make the call with the same sequence parameters.
 * Everything a call enqueues before its one host wait - the GOP steps with their exchanges, the strip's slices, the all-gather of
 * the sizes - is recorded into a hipGraph when the same shape comes a second time, and launched as one graph from then on
 * (option "strip_graph": by default with world == 1 and the single-GPU timing communicators; between the ranks of an RCCL job
 * only when asked for with 1; never with option "profile" or an in-process communicator).
 * A rank whose own work fails - a launch or an allocation refused, the output rank's d_out missing or not 16-byte aligned - keeps
 * the collective call order and marks its sizes; every rank then returns an error from the same call instead of waiting for it
 * inside an exchange.  What is rank-local and NOT covered: M2V_E_PARAM for rank / world / communicator arguments (the same on
 * every rank by construction) and M2V_E_STATE for a handle that is busy with another sequence - the caller's bug on that rank;
 * the other ranks of an RCCL job then wait for it, and the job has to be taken down (bench.py's launcher does).
 */
int m2v_strip_encode(m2v_enc *e, m2v_comm *comm, int rank, int world, int dst_rank, uint32_t xsize16, uint32_t ysize16,
                     uint32_t pframes_count, const void *d_frames444, size_t nframes, void *d_out, size_t cap, size_t *out_bytes,
                     void *hip_stream);
/*
 * The same sequence in two halves, so that ONE thread keeps two strip sequences in flight on two handles (as m2v_encode_resident_begin /
 * _end do for the whole frame): _begin enqueues the GOP steps and this strip's slices and returns; _end issues the all-gather of the sizes,
 * does the one host wait, sends / receives the strips and, on the output rank, assembles the stream; when it returns on the output rank
 * the handle's stream is synchronised, d_out is complete and *out_bytes holds the byte count.  On the other ranks (*out_bytes = 0) the
 * strip may still be on its way to the output rank: the handle's next call is ordered behind it on its stream (m2v_reset and m2v_destroy
 * wait for it), and a caller-owned hip_stream has to be synchronised by the caller before it is destroyed.  Between the two calls the handle takes no other work
 * (M2V_E_STATE).  Handles that take turns each need a peer communicator of their own (landing block, arrival counters) - over ONE shared
 * base communicator: every collective of a sequence's second half is issued by _end, so the ranks issue their collectives in one and the
 * same order (begin A, begin B, end A, begin A', end B ...) and RCCL, which runs a communicator's operations in issue order whatever
 * stream each is on, never holds one sequence's strips behind another sequence's kernels.  What it hides: the host's wait for the sizes,
 * the sizes exchange and, on the output rank, the gather and the final assembly - all of it beside the other sequence's kernels.
 * Slices are independent (RTL:2704-2715), GOPs closed (RTL:2656): nothing in the stream depends on how many sequences are under way.
 */
int m2v_strip_encode_begin(m2v_enc *e, m2v_comm *comm, int rank, int world, int dst_rank, uint32_t xsize16, uint32_t ysize16,
                           uint32_t pframes_count, const void *d_frames444, size_t nframes, void *d_out, size_t cap, void *hip_stream);
int m2v_strip_encode_end(m2v_enc *e, size_t *out_bytes);

/* Timings of the last m2v_strip_encode on this handle: host microseconds per GOP step and how much of that was spent inside the
 * communicator (RCCL: enqueueing; a local communicator blocks there until the neighbour thread has posted) - always - and, with
 * option "profile", the GPU-event times in ms: halo_total (edge rows packed .. neighbour rows there, summed over the steps),
 * halo_exposed (interior rows done .. neighbour rows there), gather (from the strip's own slices being assembled: sizes + strips
 * to the output rank + final assembly).  Returns the step count. */
int m2v_strip_stats(const m2v_enc *e, double *halo_total_ms, double *halo_exposed_ms, double *gather_ms, double *host_us_per_step,
                    double *comm_us_per_step);

/* How the last m2v_strip_encode on this handle ran its GOP steps: 0 = enqueued call by call, 1 = one recorded hipGraph, 2 = the peer
 * form (one launch per step, rows stored into the neighbours' landing blocks); after a fallback inside the call: what the second attempt was. */
int m2v_strip_last_form(const m2v_enc *e);

/* The recorded-graph side of m2v_strip_encode on this handle: whether the last call was launched as a graph, recordings and graph
 * launches so far.  Returns 1 if recording has failed on this handle (the sequence is then enqueued call by call), else 0. */
int m2v_strip_graph_stats(const m2v_enc *e, int *last_call_was_graph, int *recordings, int *launches);

/* Options: "batch_frames" (frames buffered before the GPU is kicked, default 96; 1 .. 65536, M2V_E_PARAM beyond),
 * "profile" (1 = time the launches with HIP events: one interval per run of consecutive launches of one kernel on one stream),
 * "async" (default 1: the port path keeps two chunks in flight - while one chunk is uploaded, encoded and
 * read back, m2v_push_* fills the pinned staging of the next one; 0 = a chunk is complete when the push
 * that filled it returns.  The bytes are the same either way),
 * "copy_threads" (default 8: threads m2v_push_frames uses to copy large inputs into pinned memory),
 * "direct_upload" (default 1: frames handed to m2v_push_frames in page-locked host memory - hipHostMalloc / hipHostRegister -
 * are uploaded straight from the caller's buffer, without the copy into the handle's pinned staging; the call returns when
 * the upload of its frames has completed, the encoding continues asynchronously.  The same holds for m2v_push_packed (the packed
 * bytes go up as they are and are de-interleaved on the device) and for whole frames of m2v_push_beats on three page-locked arrays
 * (one strided copy per plane); these two always return with their bytes read.  2 = the same with the completion DEFERRED: the
 * call returns while its frames are still being read, and what it waits for is the PREVIOUS call's upload - the caller keeps a
 * pushed range unchanged until the next m2v_push_frames, m2v_sequence_stop or m2v_upload_wait on the handle has returned; the copy
 * engine then always has the next transfer queued behind the running one, which is what a single caller needs to keep the link
 * busy.  0 = always through the staging copy),
 * "split_streams" (default 2; 1..8 = the closed GOPs of a chunk are encoded as this many independent groups on as many
 * HIP streams, so that the partially filled tail of one group's launch overlaps with another group's next launch;
 * 1 = a single stream; ignored while "profile" is on, which times every launch with in-band events on one stream),
 * "dct_mfma" (default 1: the four luma tiles' 2-D DCT runs on the matrix cores as two chained i8 GEMMs,
 * B16 . Z . B16^T with the 19-bit intermediate in three byte limbs; 0 = every tile on the integer v_dot4 / v_mad_i32_i24
 * path through LDS.  Bit-identical results either way; the default is the faster one under rocprofv3),
 * "stream_priority" (-1 low, 0 normal, 1 high; only while idle: the handle's own stream is created again at that priority.  HIP keeps the hardware
 * queues of different priorities apart, so two handles of different priorities never share one - see bench.py's queue placement check),
 * "cu_pack" (default 5; 0..8: which macroblocks tend to share a CU in time - see xcd_remap in csrc/m2v_kernels.hpp; 0 = none.  Same bytes),
 * "strip_graph" (default -1 = automatic: m2v_strip_encode launches its sequence as a recorded hipGraph with world == 1 and with the
 * single-GPU timing communicators, call by call between the ranks of an RCCL job; 1 = recorded wherever the communicator can be
 * recorded - cross-rank RCCL included, which no hardware run has covered yet -; 0 = always call by call),
 * "conformant" (default 0 = the reference's arithmetic, byte-identical to the RTL.  1 = NOT the reference's
 * behaviour: the reconstruction loop follows ISO/IEC 13818-2 where the RTL deviates from it - four-sample average
 * rounded with +2, 4:2:0 chroma vector = mv / 2 toward zero, inverse quantiser truncating toward zero with
 * [-2048, 2047] saturation and mismatch control - so that a standard decoder reproduces the encoder's reference
 * frames exactly instead of drifting inside a GOP.  Only while idle),
 * "stats" (default 0 = exactly the launches, buffers and bytes of a handle that never heard of it.  1 = every picture leaves a
 * record for m2v_picture_stats, see there: the same stream, one reconstruction more per GOP and a pass over source and reconstruction
 * per GOP step.  Only while idle, M2V_E_STATE otherwise),
 * "gop_bytes_max" (default 0 = off.  B > 0 = NOT the module's behaviour: a byte cap per GOP, held on the device - see m2v_gop_report.
 * Only while idle, M2V_E_STATE otherwise; a negative value is M2V_E_PARAM),
 * "scene_cut" (default 0 = off.  T = 1..65280 = NOT the module's behaviour: a GOP starts where the device finds a scene cut - see
 * m2v_set_gop_starts.  Only while idle, M2V_E_STATE otherwise; a value outside 0..65280 is M2V_E_PARAM). */
int m2v_set_option(m2v_enc *e, const char *name, long long value);

/*
 * A level per GOP.  NOT the module's behaviour (like option "conformant" and M2V_HEADER_TRUE): the module takes Q_LEVEL as a
 * parameter and holds it for good.  The stream stays a legal one: the level appears in one place only, the quantiser_scale_code of
 * every slice header (2 << level as the 5-bit code's value, RTL:2708-2710), which ISO/IEC 13818-2 lets change from slice to slice; the
 * sequence header does not depend on it; and GOPs are closed, so a GOP coded at level q is, byte for byte, that GOP of the same clip
 * encoded whole at Q_LEVEL = q.
 *
 * m2v_set_gop_levels: GOP k of every sequence STARTED afterwards is coded at levels[min(k, n - 1)], k = frame number /
 * (pframes_count + 1).  Values are 1..4; anything else answers M2V_E_PARAM and the previous setting stays.  n == 0 or levels == NULL
 * clears the setting (every GOP at the handle's Q_LEVEL again).  Entries past the sequence's last GOP are ignored.  The array is
 * copied: it is the caller's again on return.  The setting is sampled when a sequence starts (where xsize16 / ysize16 /
 * pframes_count are), stays until it is changed and survives m2v_reset.  It holds for the port path and every resident entry, for
 * any "batch_frames" and "split_streams" (a GOP that continues in the next chunk keeps its level).  A schedule whose every used entry
 * equals Q_LEVEL gives exactly the launches and the stream of a handle without one.  While a schedule or a cap is set every
 * m2v_strip_* entry that starts something answers M2V_E_STATE - the rule "stats" and a set frame size follow.
 */
int m2v_set_gop_levels(m2v_enc *e, const uint8_t *levels, size_t n);

/*
 * Option "gop_bytes_max" = B > 0, resident entries (m2v_encode_resident*, also _begin / _end).
 * The size of a GOP is its bytes in the stream, from its group_start_code (00 00 01 B8) up to the next one or to the
 * sequence_end_code: the headers of its pictures (25 bytes for the I picture with the GOP header, 18 for a P picture) plus the bytes
 * of their slices.  The sequence header is not part of GOP 0, the end code and the final padding not of the last one.  A sequence header
 * repeated in front of a later GOP (repeat_headers of m2v_set_stream_desc) is not part of any GOP either: neither bytes nor the cap count it.
 * GOP k is coded at the smallest level q >= start_k whose size is <= B; if none is, at 4.  start_k is the schedule's entry for k
 * (m2v_set_gop_levels), or the handle's Q_LEVEL without a schedule.  The search goes upwards one level at a time and stops at the
 * first fit, so "smallest" is well defined even where sizes are not monotone in q.  The result depends on the clip alone: not on
 * "batch_frames", "split_streams" or "cu_pack".
 * A chunk has to hold whole GOPs: with pframes_count + 1 > "batch_frames" the call that starts the sequence answers M2V_E_PARAM.
 * The GOPs over the cap are encoded again on the device, up to three more times; the host waits for the device's verdict after each
 * try (at most three waits per chunk, and only with the option on).  m2v_encode_resident*_begin does these waits INSIDE _begin: with
 * the cap on, _begin returns with the sequence's last chunk enqueued, not with nothing waited for.
 * The m2v_push_* calls that start a sequence answer M2V_E_STATE while the cap is set (the schedule does work there).
 * With "stats" on, the picture records of a GOP that went again are those of its final level.
 */
typedef struct m2v_gop_stat {
    uint32_t gop;            /* index of the GOP in its sequence                                             */
    uint32_t first_frame;    /* its first picture, and how many it has (the last GOP may be cut short)       */
    uint32_t frames;
    uint32_t level;          /* the level it is coded at in the stream, 1..4                                  */
    uint64_t bytes;          /* its size at that level, as defined above                                      */
    uint32_t tries;          /* encodes of this GOP, 1..4                                                     */
    uint32_t over;           /* 1 = even the final size exceeds B (level is then 4)                           */
} m2v_gop_stat;              /* 32 bytes */
/* Pops up to `cap` records, oldest first, into dst and returns how many it wrote; dst == NULL returns how many are waiting.  After
 * m2v_encode_resident* or m2v_encode_resident_end has returned one record per GOP of that sequence is waiting.  Records still
 * unread when the next sequence starts, or at m2v_reset, are dropped.  A sequence coded with the cap off leaves none: the answer is 0.
 * Waits for nothing. */
long long m2v_gop_report(m2v_enc *e, m2v_gop_stat *dst, size_t cap);

/*
 * Where GOPs start.  NOT the module's behaviour (like option "conformant" and a level per GOP): the module starts a GOP every
 * pframes_count + 1 frames, counted from frame 0.  The stream stays a legal one: GOPs are closed, an I picture resets
 * temporal_reference, and the GOP header's time code is a function of the frame number alone - so a GOP [s, s + L) is, byte for byte,
 * GOP 0 of the frames s .. s + L - 1 encoded alone, with the time code of frame s.
 *
 * The rule.  With pf = pframes_count & 0xFF and s = the frame number of the I picture of the GOP in progress, frame n starts a GOP
 * iff any of these holds:
 *   M2V_GOP_FIRST    n = 0
 *   M2V_GOP_CADENCE  n - s = pf + 1
 *   M2V_GOP_LIST     n is in the caller's list (m2v_set_gop_starts)
 *   M2V_GOP_CUT      option "scene_cut" is on and the detector flags n
 * The cadence counts from the last I picture, whatever caused it: no GOP is longer than pf + 1.  The picture's place in its GOP is
 * n - s, and a level schedule (m2v_set_gop_levels) goes by the GOP's ordinal, the count of GOP starts before n.  With neither list nor
 * detector that is n / (pf + 1), and the launches and the stream are exactly those of a handle that never heard of either.
 *
 * m2v_set_gop_starts: the list, strictly ascending frame numbers; anything else answers M2V_E_PARAM and the previous setting stays.
 * n == 0 or frames == NULL clears it.  The list is copied, sampled when a sequence starts (where xsize16 / ysize16 / pframes_count and
 * the level schedule are), stays until changed and survives m2v_reset.  Entries past the sequence's end are ignored, and 0 and
 * cadence positions change nothing.  It holds on the port path and on every resident entry, for any "batch_frames", "split_streams",
 * "stats", "conformant", input format and set frame size.
 *
 * m2v_gop_layout: the rule as plain arithmetic (no GPU, no handle; the function the encoder itself plans with): writes the reasons
 * (M2V_GOP_FIRST / CADENCE / LIST, never CUT) of each of nframes frames to flags_out (may be NULL) and returns the number of GOPs;
 * M2V_E_PARAM for a list that is not strictly ascending.
 *
 * Option "scene_cut" = T, 1..65280, resident entries.  Integers only: S_n(mb) = the sum of the 256 luma samples of macroblock mb of
 * picture n AS CODED - after the 4:2:0 expansion or RGB conversion, padding of a set frame size included; D(n) = the sum over all
 * macroblocks of |S_n - S_(n-1)| for n >= 1, D(0) = 0; frame n is flagged iff D(n) > T * (macroblocks of a picture).  In words: the
 * macroblocks' mean luma moved by more than T / 256 grey levels on average.  The result depends on the pictures alone, not on
 * "batch_frames" or "split_streams".  Per chunk the host waits once for the device's flags before it plans the chunk (only with the
 * option on); m2v_encode_resident*_begin does these waits INSIDE _begin, as with the cap.
 *
 * Refusals (m2v_last_error names the reason): an m2v_push_* call that starts a sequence while "scene_cut" is set answers M2V_E_STATE
 * (the list does work there); every m2v_strip_* entry that starts something while a list or "scene_cut" is set answers M2V_E_STATE;
 * a sequence that starts with "gop_bytes_max" set together with a list or "scene_cut" answers M2V_E_STATE with nothing started (the
 * cap judges GOPs of the fixed cadence).
 */
enum { M2V_GOP_FIRST = 1, M2V_GOP_CADENCE = 2, M2V_GOP_LIST = 4, M2V_GOP_CUT = 8 };
int m2v_set_gop_starts(m2v_enc *e, const uint32_t *frames, size_t n);
long long m2v_gop_layout(uint32_t pframes_count, const uint32_t *starts, size_t n, size_t nframes, uint8_t *flags_out);
typedef struct m2v_scene_stat {
    uint32_t frame;          /* index of the picture in its sequence                                          */
    uint32_t flags;          /* M2V_GOP_*: every reason that applies; the picture starts a GOP iff flags != 0  */
    uint64_t diff;           /* D(n) as defined above; 0 with the detector off                                */
} m2v_scene_stat;            /* 16 bytes */
/* Pops up to `cap` records, oldest first, into dst and returns how many it wrote; dst == NULL returns how many are waiting: one per
 * picture of a sequence that had a list or the detector, none otherwise.  They arrive as m2v_picture_stats' records do, are dropped
 * when the next sequence starts and at m2v_reset.  Waits for nothing. */
long long m2v_scene_report(m2v_enc *e, m2v_scene_stat *dst, size_t cap);

/*
 * Per-picture statistics, computed on the device while a chunk is encoded (option "stats" = 1): the squared error of the
 * reconstruction against the source, the bits of the macroblock layer and the macroblock decisions.
 *
 * Source: the 4:2:0 picture the module codes - Y as given, U and V after the module's own two-stage mean2 (RTL:1086-1089 the
 * horizontal mean of a pixel pair, RTL:1167-1170 the vertical mean of two such means, each (a + b + 1) >> 1).  For 4:2:0 and RGB
 * input that is taken after the expansion or conversion the handle does anyway.  A frame cut short by a stop counts with its black
 * fill (Y = 0, U = V = 128, RTL:1048-1056), as it is coded.
 * Reconstruction: what the module's reference memory would hold for the picture (every picture, the unreferenced last one of a GOP
 * included).  With option "conformant" = 1 that is also the picture a standard decoder shows.  WITHOUT it a standard decoder drifts
 * away from it inside a GOP (see "conformant"): the records then say how well the MODULE's loop tracked the source, not what a
 * player displays; only the I pictures agree.
 * Measured region: without a frame size set the whole coded W x H of luma and W/2 x H/2 of each chroma plane.  With
 * m2v_set_frame_size(width, height, ...) the top-left width x height of luma and (width + 1) / 2 x (height + 1) / 2 of each
 * chroma plane: the padding is coded, and not measured.
 * Arithmetic: exact integers throughout, no float on the device, so a record does not depend on the launch shape, on "batch_frames",
 * "split_streams" or "cu_pack".  PSNR is the caller's: 10 log10(255^2 * samples / sse), infinite for sse == 0.
 *
 * While "stats" is 1 every m2v_strip_* entry that starts something answers M2V_E_STATE (a strip holds part of a picture per GPU;
 * nothing sums across ranks) - the rule a set frame size follows.
 */
typedef struct m2v_picture_stat {
    uint32_t frame;          /* index of the picture in its sequence, 0-based (coding order = display order) */
    uint32_t coding_type;    /* 1 = I, 2 = P, as m2vc_picture                                               */
    uint64_t sse[3];         /* Y, U, V: sum over the measured region of (source - reconstruction)^2         */
    uint64_t mb_bits;        /* bits of the macroblock layer of the picture (slice headers not counted)      */
    uint32_t intra_mbs, inter_mbs;
    uint32_t coded_blocks;   /* sum over macroblocks of popcount(coded block flags), 0 .. 6 each             */
    uint32_t mv_abs_x, mv_abs_y;   /* sum over inter macroblocks of |vector| as transmitted, half-pel units  */
    uint32_t reserved;       /* 0 */
} m2v_picture_stat;          /* 64 bytes */
/* Pops up to `cap` records of completed pictures, oldest first, into dst and returns how many it wrote; dst == NULL returns how
 * many are waiting.  After m2v_encode_resident* or m2v_encode_resident_end has returned all nframes records of that sequence are
 * waiting.  On the port path a chunk's records arrive when m2v_pull could hand out that chunk's words; after the stop has been
 * pulled to `last`, all of them have.  Records still unread when the next sequence starts, or at m2v_reset, are dropped.  With
 * "stats" = 0 the answer is 0.  Waits for nothing. */
long long m2v_picture_stats(m2v_enc *e, m2v_picture_stat *dst, size_t cap);

/*
 * Reconstructed pictures out: every coded picture of a resident sequence as a plain 4:2:0 frame in a device buffer of the caller's.
 *
 * m2v_set_recon_out(e, d_dst, cap, layout): frame n of every sequence started afterwards by a resident entry (m2v_encode_resident,
 * m2v_encode_resident420, m2v_encode_resident_rgb, each also as _begin / _end) is written to d_dst + n * frame_bytes in `layout`
 * (M2V_420_I420 / YV12 / NV12 / NV21), n being the frame's number from the sequence's start.
 * What is written: the picture the module's reference memory would hold for that frame - what m2v_picture_stats measures against -
 * for every picture, the ones no P picture refers to included (the last of every GOP; every one with pframes_count = 0).  With option
 * "conformant" = 1 it is byte for byte the picture a standard decoder shows.  WITHOUT it a standard decoder drifts away from it inside a
 * GOP (see "conformant"): the frames then show the MODULE's loop, not what a player displays.
 * Frame size: without a frame size set W x H of luma and W/2 x H/2 of each chroma plane, frame_bytes = W * H * 3 / 2.  With
 * m2v_set_frame_size(width, height, ...) the top-left width x height of luma and cw x ch = (width + 1) / 2 x (height + 1) / 2 of each
 * chroma plane, frame_bytes = width * height + 2 * cw * ch: the cropped picture a player of an M2V_HEADER_TRUE stream displays, and the
 * region "stats" measures.  Either way the frames are packed exactly as frames of that size and layout are on the way in: rows of
 * width (cw, or interleaved 2 * cw) bytes without padding, frame behind frame.  d_dst needs no alignment.  No byte outside
 * [n * frame_bytes, (n + 1) * frame_bytes) of a coded frame n is touched.
 * When the data is complete: the writes are ordered on the call's stream - complete when the blocking call or _end has returned, and
 * for work queued on that stream afterwards.  The buffer stays the caller's and must stay valid until then.
 * The setting is sampled when a sequence starts (where a frame size and a level schedule are), stays until changed and survives
 * m2v_reset; d_dst == NULL clears it.  Only while idle, M2V_E_STATE otherwise; a layout outside 0..3 is M2V_E_PARAM.  A sequence start
 * whose nframes * frame_bytes exceeds cap answers M2V_E_OVERFLOW before anything is launched.
 * The stream is byte for byte the stream without the setting, and with no buffer set the launches, buffers and plan are exactly
 * those of a handle that never heard of it.  With one set every picture keeps a reconstruction slot (one more per GOP, as with
 * "stats") and one kernel per GOP step moves 3 bytes per pixel.  It goes with "stats", m2v_set_gop_levels, "gop_bytes_max" (a GOP that
 * is coded again leaves the frames of its final level), m2v_set_gop_starts, "scene_cut", any "batch_frames" and "split_streams",
 * "conformant", every input format and a set frame size.
 * Refusals: while a buffer is set every m2v_push_* call that starts a sequence answers M2V_E_STATE (a read-back over the link is another
 * feature), and so does every m2v_strip_* entry that starts something - the rule "stats" follows.
 */
int m2v_set_recon_out(m2v_enc *e, void *d_dst, size_t cap, int layout);   /* layout: M2V_420_I420 | YV12 | NV12 | NV21 */

/*
 * What the stream says about itself.  NOT the module's behaviour (like option "conformant", M2V_HEADER_TRUE, a level per GOP and GOP
 * starts): the module hard-wires the 34 bytes of its sequence headers (RTL:2598-2617) and counts its time code at 24 frames per second
 * (RTL:2685-2698).  With a description set the stream stays a legal ISO/IEC 13818-2 one; with none, or one equal to the module's, the
 * stream, the launches and the kernel arguments' values are the module's.
 *
 * The bytes.  The 34 bytes of sequence_header + sequence_extension + sequence_display_extension with these fields substituted, widths in
 * order:  sequence_header 32, 12, 12, 4 aspect, 4 rate, 18 bit rate low, marker, 10 vbv low, 3 zero;  sequence_extension 32, 4 = 1,
 * 8 = 0x44, 1 = 0, 2 = 1, 4 zero, 12 bit rate high, marker, 8 vbv high, 8 zero;  sequence_display_extension 32, 4 = 2, 3 video_format,
 * 1 = 1, 8, 8, 8 colour, 14 display width, marker, 14 display height, zero bits to the byte.  profile_and_level, progressive_sequence,
 * low_delay, frame_rate_extension_n / _d and the matrix flags do not change.
 * The time code of frame n (the four bytes behind every 00 00 01 B8): with F = 24, 24, 25, 30, 30, 50, 60, 60 for frame_rate_code 1..8
 * it is the module's formula with 24 replaced by F - pictures = n mod F, seconds = (n / F) mod 60, minutes = (n / 60F) mod 60, and the six
 * bits the module writes in front hold min(n / 3600F, 63): the module's saturation, and its spill into drop_frame_flag from 32 hours on.
 * Then the marker, closed_gop = 1, broken_link = 0.  Code 2 gives the module's bytes.  There is no true drop-frame counting.
 * repeat_headers = 1: the same 34 bytes, printed and display sizes included, also stand in front of the group_start_code of every GOP
 * after the first, whatever started it - cadence, m2v_set_gop_starts or "scene_cut" (ISO 6.1.1.6 allows it): a player can start at any
 * GOP.  m2v_gop_stat.bytes and the cap's verdict do not count them, mb_bits of "stats" is untouched.
 *
 * m2v_set_stream_desc: any field out of range, one display size zero and the other not, reserved != 0 or repeat_headers > 1 answers
 * M2V_E_PARAM and the previous setting stays.  d == NULL sets the module's values again.  Only while the handle is idle, M2V_E_STATE
 * otherwise (between _begin and _end, during a port sequence).  The structure is copied, sampled when a sequence starts (where a level
 * schedule is), stays until changed and survives m2v_reset.  It holds on every whole-frame path - the port path in all its forms and
 * every resident entry - with any "batch_frames", "split_streams", "stats", "conformant", input format, set frame size, level schedule,
 * "gop_bytes_max", GOP list, "scene_cut" and m2v_set_recon_out.  While a description that differs from the module's is set every
 * m2v_strip_* entry that starts something answers M2V_E_STATE - the rule "stats", a frame size, a schedule and a list follow.
 */
typedef struct m2v_stream_desc {
    uint32_t frame_rate_code;           /* 1..8, table 6-4                                        module: 2     */
    uint32_t aspect_ratio_information;  /* 1..4, table 6-3                                        module: 1     */
    uint32_t bit_rate_400;              /* 1..2^30-1, units of 400 bit/s: low 18 bits in
                                           sequence_header, high 12 in sequence_extension         module: 10000 */
    uint32_t vbv_buffer_size_16k;       /* 0..2^18-1, units of 16384 bits: low 10 / high 8 bits   module: 0     */
    uint32_t video_format;              /* 0..5                                                   module: 1     */
    uint32_t colour_primaries;          /* 1..255 (0 is forbidden)                                module: 5     */
    uint32_t transfer_characteristics;  /* 1..255                                                 module: 5     */
    uint32_t matrix_coefficients;       /* 1..255                                                 module: 5     */
    uint32_t display_width;             /* both 0 = the size sequence_header prints (today's rule, M2V_HEADER_TRUE */
    uint32_t display_height;            /* included); else both 1..16383                                           */
    uint32_t repeat_headers;            /* 0 | 1                                                  module: 0     */
    uint32_t reserved;                  /* 0 */
} m2v_stream_desc;                      /* 48 bytes */
void m2v_stream_desc_module(m2v_stream_desc *d);                 /* the module's values */
int m2v_set_stream_desc(m2v_enc *e, const m2v_stream_desc *d);   /* NULL = the module's again */
/* 1..8 for a rational EQUAL to one of table 6-4 (30000/1000 is 30), else M2V_E_PARAM.  Plain arithmetic. */
int m2v_frame_rate_code(uint32_t num, uint32_t den);
/* the four bytes behind 00 00 01 B8 for frame n at frame_rate_code 1..8 (M2V_E_PARAM otherwise): the function the encoder prints; no GPU,
 * no handle */
int m2v_time_code(uint32_t frame_rate_code, uint32_t n, uint8_t out[4]);

/*
 * A batch of sequences in one resident call: one stream per clip.  NOT the module's behaviour as a call - the module codes one sequence -
 * but every stream in the output is the module's: with the setting, the bytes at [off[b], off[b + 1]) of d_out are the stream of clip b
 * encoded alone by m2v_encode_resident with the same handle settings.
 *
 * m2v_set_sequences(e, frames_per_sequence, n): the frames of every resident call started afterwards are n clips, clip b being the
 * frames [F_b, F_b + L_b) of the call with L_b = frames_per_sequence[b] and F_b the sum of the entries before it.  NULL or n == 0
 * clears the setting.  The list is copied, sampled when a call starts (where the list of m2v_set_gop_starts is), stays until changed and
 * survives m2v_reset.  Only while idle, M2V_E_STATE otherwise.  Every resident entry takes it - m2v_encode_resident,
 * m2v_encode_resident420, m2v_encode_resident_rgb, blocking and as _begin / _end.  The call's nframes must equal the sum of the
 * entries and no entry may be 0: otherwise the call answers M2V_E_PARAM before anything of the handle changes.  A list of ONE entry
 * samples as "none": the plan, the launches, the kernel arguments' values and the stream are exactly those of a handle with nothing set.
 *
 * Clip b: its first frame is an I picture and frame number 0 - time codes, temporal_reference, the cadence pframes_count + 1, the
 * ordinal a level schedule (m2v_set_gop_levels) goes by and m2v_picture_stat.frame all count from F_b.
 * Layout: off[0] = 0, off[b + 1] = off[b] + len_b, where len_b follows the module's final-word rule applied to the clip alone:
 * ((B + 4) / 32 + 1) * 32 for B bytes in front of its sequence_end_code (RTL:2621-2628, 2932-2937).  Every stream therefore starts on a
 * 32-byte boundary; its sequence headers (with the description of m2v_set_stream_desc, and with repeat_headers in front of each of its
 * later GOPs too) stand in front of its first frame, and its sequence_end_code and zero padding end it.  *out_bytes is off[n];
 * cap < off[n] answers M2V_E_OVERFLOW as ever.
 * It holds with every input format, a set frame size, "conformant", a level schedule, a stream description, any "batch_frames" and
 * "split_streams" (a chunk may cut a clip anywhere, hold many clips, and a clip may span several chunks), "stats" (the records are those
 * of each clip alone, in batch order) and m2v_set_recon_out (frame n OF THE CALL lands at n * frame_bytes).
 *
 * m2v_sequence_report: pops up to `max` records, oldest first, into out and returns how many it wrote; out == NULL returns how many are
 * waiting.  After a call with the setting (or its _end) has returned, one record per clip is waiting: offset = off[b], bytes = len_b,
 * first_frame = F_b, frames = L_b, gops = GOPs of the clip.  The device writes them into pinned memory with the scan of every chunk, they
 * are complete where the control word is: no wait is added.  Dropped when the next call starts and at m2v_reset.
 *
 * Refusals (M2V_E_STATE, m2v_last_error names the reason) while a list is set: every m2v_push_* call that starts a sequence, every
 * m2v_strip_* entry that starts something, and a resident call that starts with a list of two or more entries together with
 * m2v_set_gop_starts, "scene_cut" or "gop_bytes_max".  Their host sides count one sequence: these are the follow-ups.
 */
int m2v_set_sequences(m2v_enc *e, const uint32_t *frames_per_sequence, size_t n);   /* NULL / 0: none */
typedef struct m2v_sequence_stat { unsigned long long offset, bytes; uint32_t first_frame, frames; uint32_t gops, reserved; } m2v_sequence_stat;  /* 32 bytes */
int m2v_sequence_report(m2v_enc *e, m2v_sequence_stat *out, size_t max);   /* returns the count, like m2v_gop_report */

/*
 * Transport and program stream out of the resident call, muxed on the device.  The bytes are exactly those m2vc_mux_ts / m2vc_mux_ps
 * (include/m2v_container.h) return for the same elementary stream - csrc/m2v_container.cpp is the specification: the zero padding after
 * sequence_end_code is dropped, the sequence headers travel in picture 0's PES packet, a repeated sequence header opens its GOP's access
 * unit, PTS = pts0 + i * 90000 * den / num with the frame rate the stream states, the same rates, PAT / PMT, PCR, stuffing, packs, SCR and
 * system header.  File playback only, as there: nothing is paced against the T-STD / P-STD buffer models.
 *
 * m2v_set_mux_out(e, kind, d_dst, cap): every resident call started afterwards (m2v_encode_resident, m2v_encode_resident420,
 * m2v_encode_resident_rgb, each also as _begin / _end) also leaves its stream as a container of `kind` in the `cap` bytes of device memory
 * at d_dst (no alignment needed).  Three kernels follow the last chunk's assembly on the call's stream and take the stream's length
 * from the device: no wait is added, and the data is complete where the stream is - when the blocking call or _end has returned, and for
 * work queued on that stream afterwards.  The elementary stream in d_out is byte for byte what it is without the setting, and with
 * nothing set the launches are exactly those of a handle that never heard of it.  With m2v_set_sequences there is one container per clip:
 * container 0 starts at d_dst, container b at the next multiple of 32 bytes after the end of container b - 1; the gaps are not touched.
 * Nothing past cap is ever written, and a stream whose status is not M2V_MUX_OK writes nothing at all.
 * It holds with a frame size, "conformant", levels per GOP, "gop_bytes_max" (the mux runs once, after the final redo), GOP starts,
 * "scene_cut", "stats", m2v_set_recon_out, a stream description (its frame_rate_code sets the PTS step; with repeat_headers a player
 * can join the transport stream at any GOP), any "batch_frames", "split_streams" and input format.
 * The setting is sampled when a call starts, stays until changed and survives m2v_reset; kind = M2V_MUX_NONE clears it.  Only while idle,
 * M2V_E_STATE otherwise; an unknown kind, or a kind with d_dst == NULL, is M2V_E_PARAM.  While a buffer is set every m2v_push_* call that
 * starts a sequence and every m2v_strip_* entry that starts something answers M2V_E_STATE - the rule m2v_set_recon_out follows - and a
 * batch of more than 65535 clips answers M2V_E_PARAM when the call starts.
 *
 * m2v_mux_report: pops up to `max` records, oldest first, into out and returns how many it wrote; out == NULL returns how many are
 * waiting.  After a call with the setting (or its _end) or m2v_mux_device has returned, one record per stream is waiting: where the
 * elementary stream is in its buffer, where the container is in d_dst (out_bytes = 0 unless status is M2V_MUX_OK), the pictures, and
 * status = M2V_MUX_OK, M2V_MUX_SYNTAX (not a stream as this encoder writes it: it does not begin with a sequence header, a picture is
 * neither I nor P, something other than zeros follows the end code, the frame_rate_code is reserved, there is no picture) or
 * M2V_MUX_OVERFLOW (the container does not fit what is left of cap: it takes no room, and a later one of the call that fits is
 * written where it would have started - or the elementary stream itself overflowed d_out: then every record says so).  The device writes them into pinned memory; no wait is added.  Dropped when the next
 * resident call starts, at the next m2v_mux_device and at m2v_reset.
 *
 * m2v_mux_device: the same kernels over nstreams streams already in device memory - stream i is the es_bytes[i] bytes at
 * d_es + es_off[i], at any byte alignment (port-path output, a strip result, a splice); es_off / es_bytes are host arrays.  The call
 * blocks (hip_stream or the handle's stream is waited for), the records come through m2v_mux_report, and the function's own answer is
 * M2V_OK whenever the kernels ran.  M2V_E_STATE while a sequence is in progress or a resident call in flight; at most 65535 streams.
 *
 * m2v_mux_bound(kind, es_bytes, pictures): a capacity that always suffices for a stream of es_bytes bytes (padding included) and
 * `pictures` pictures; 0 for an unknown kind.  From the packet geometry:
 *   TS  a picture of b bytes is a PES packet of 14 + b bytes; its first transport packet carries 176 of them behind the PCR, every other
 *       one 184: 1 + ceil((b - 162) / 184) <= b / 184 + 2 packets.  A PAT / PMT pair precedes a picture at most: 2 more.  Over all
 *       pictures: 188 * (es_bytes / 184 + 4 * pictures + 1).
 *   PS  a picture's first pack spends 28 bytes on pack and PES header with PTS, every further one (each carries 2025 bytes) 23:
 *       at most 28 + 23 * (b / 2025 + 1) a picture; 15 for the system header and 4 for MPEG_program_end_code once:
 *       es_bytes + 23 * (es_bytes / 2025) + 51 * pictures + 19.
 * For a batch add 31 bytes per clip for the 32-byte boundaries.
 *
 * m2v_mux_scan_tile: the byte span after which the start-code scan hands over to another workgroup (a test aims headers at its multiples).
 */
enum { M2V_MUX_NONE = 0, M2V_MUX_TS = 1, M2V_MUX_PS = 2 };
enum { M2V_MUX_OK = 0, M2V_MUX_SYNTAX = -2, M2V_MUX_OVERFLOW = -3 };      /* the values of M2VC_E_SYNTAX / M2VC_E_OVERFLOW */
typedef struct { uint64_t es_offset, es_bytes, out_offset, out_bytes; uint32_t pictures; int32_t status; } m2v_mux_stat;   /* 40 bytes */
size_t m2v_mux_bound(int kind, size_t es_bytes, size_t pictures);
int m2v_set_mux_out(m2v_enc *e, int kind, void *d_dst, size_t cap);
int m2v_mux_report(m2v_enc *e, m2v_mux_stat *out, size_t max);   /* returns the count, like m2v_sequence_report */
int m2v_mux_device(m2v_enc *e, int kind, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams, void *d_dst,
                   size_t cap, void *hip_stream);
int m2v_mux_scan_tile(void);

/*
 * Decode on the device: an MPEG-2 elementary stream of this encoder's syntax back to plain 4:2:0 frames, without the stream or the frames
 * leaving HBM.  NOT part of the module's behaviour.  The definition is fpga-mpeg2-encoder_amd/decoder.py, as m2v_container.cpp is for the
 * device muxer: for a stream that decoder.decode(data, quirks) reads, the device writes every picture in stream order, frame n at
 * d_dst + n * frame_bytes, cropped to the w x h of the sequence header (chroma (w + 1) / 2 x (h + 1) / 2), rows without padding, in the
 * packing of m2v_set_recon_out (layout = M2V_420_I420 / YV12 / NV12 / NV21; frame_bytes = w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2)); the
 * bytes equal decoder.decode(...).frames.  mode:
 *   M2V_DEC_ISO     quirks = False: clause 7 of ISO/IEC 13818-2 - saturation to [-2048, 2047] and mismatch control, chroma vector / 2
 *                   toward zero, + 2 rounding of the four-sample mean, Chen-Wang with the -256 .. 255 clip: the pictures of a stream
 *                   coded with option "conformant" = 1
 *   M2V_DEC_MODULE  quirks = True: the module's own loop, as the four deviations in decoder.py's docstring state it: the pictures of the
 *                   module's streams (what m2v_set_recon_out writes while encoding)
 *
 * m2v_decode_device(e, d_es, es_bytes, d_dst, cap, layout, mode, hip_stream): d_es and d_dst are device pointers at ANY byte address;
 * d_dst is write-only and at most cap bytes of it are written, whatever the status.  The call blocks (hip_stream or the handle's stream
 * is waited for: once for the plan - picture count, size, picture types - and once at the end); its own answer is M2V_OK whenever the
 * kernels ran, and the verdict is in the record (m2v_decode_report: the last call's).  The handle's XL / YL play no part: picture sizes go
 * up to 2048 x 2048.  d_dst == NULL is a probe: only the scan and the plan run, nothing is written, cap is not looked at, and the record
 * carries pictures, width, height, frame_bytes (and out_bytes = pictures * frame_bytes, the room a decode needs).
 * M2V_E_STATE while a sequence is in progress or a resident call is in flight; M2V_E_PARAM for an unknown layout or mode.
 *
 * The record:
 *   status            M2V_DEC_OK; M2V_DEC_SYNTAX: a stream decoder.decode refuses with any exception - every check of its headers, "vector
 *                     points outside the picture", "coefficient index beyond 63", an invalid code, data that ends early, anything but zero
 *                     padding behind sequence_end_code, a length that is no multiple of 32 - or one that holds a 00 00 01 prefix anywhere
 *                     decoder.py does not read a start code (this encoder's streams hold none there); M2V_DEC_OVERFLOW: the frames do
 *                     not fit cap.  With a status other than OK out_bytes is 0; with M2V_DEC_OVERFLOW, or a syntax error found before
 *                     the first chunk's pictures are written, nothing is written at all
 *   err_offset        with M2V_DEC_SYNTAX: the byte offset of the start code of the earliest unit (header or slice) in which something
 *                     was wrong - a minimum over all units judged, so the same for every run; 0 otherwise
 *   pictures, gops, width, height, repeated_headers   what decoder.decode's result holds; chains = the number of I pictures (a chain is the
 *                     run from an I picture to the next: GOPs of I / P pictures decode independently whatever closed_gop says)
 *   es_bytes, out_bytes, frame_bytes                  the stream's length, the bytes written, the bytes of one frame
 *
 * Option "decode_batch" (m2v_set_option): pictures per chunk - the slices of a chunk's pictures are walked together, and its pictures stay
 * in the handle's buffers until they are written out.  0 (the default): as many as keep the chunk's quantised levels (768 bytes a
 * macroblock) within 256 MiB, at most 256 - 40 pictures of 1920 x 1152.  The result does not depend on it.  A larger chunk walks more
 * slices at once (the bench clip as one chunk of 90 pictures: 17 ms against 45) and holds more memory.  The buffers belong to the handle:
 * allocated by the first decode, by size, and freed with it.
 *
 * m2v_decode_scan_tile: the byte span after which the start-code scan hands over to another workgroup (a test aims start codes at its
 * multiples).
 *
 * Out of scope, and M2V_DEC_SYNTAX by the definition: B pictures, field pictures, f_codes other than 1, skipped macroblocks, quantiser
 * matrices in the stream, intra_vlc_format 1, alternate scan.  Not offered: decode on the port path or in strips.  Several streams per call:
 * m2v_decode_streams_device, below.  That is the MODULE syntax, the default; most of the list is accepted by the main syntax:
 *
 * Option "decode_syntax" (m2v_set_option), per handle: M2V_SYNTAX_MODULE (0, the default) - everything above, bit for bit and launch
 * for launch; M2V_SYNTAX_MAIN (1) - MPEG-2 Main-Profile streams of progressive frame pictures, I and P, 4:2:0, from any encoder.  The
 * definition is decoder.decode(stream, quirks=False, syntax="main") (decoder.decode_main); every stream that M2V_DEC_ISO accepts in the
 * module syntax decodes to the same frames and counts in the main syntax.  With it `mode` must be M2V_DEC_ISO (the module's four
 * deviations belong to its own syntax: M2V_DEC_MODULE is M2V_E_PARAM), and m2v_decode_streams_device returns M2V_E_STATE and touches
 * nothing.  The record, err_offset (the earliest unit the grammar refuses, else the earliest slice that cannot be read), the layouts,
 * "decode_batch" and the container path (m2v_demux_device in front) are as above.  Accepted beyond the module syntax:
 *   stream    sequence_display_extension and the GOP header are optional; repeated sequence headers, each equal to the first with
 *             its matrices, wherever a GOP or picture header may stand; user_data behind sequence_extension, GOP header and
 *             picture_coding_extension, copyright_extension and picture_display_extension behind picture_coding_extension - skipped;
 *             sequence_end_code may be missing, zero bytes may follow the last unit, the length need not be a multiple of 32 (a last
 *             picture with fewer slices than macroblock rows is refused); progressive_sequence may be anything
 *   picture   f_code[0][0] and [0][1] 1 .. 9 (15 in an I picture) with motion_residual and the wrap of 7.6.3.1; intra_dc_precision
 *             0 .. 3; q_scale_type 0 or 1 (table 7-6); alternate_scan 0 or 1 - each may change from picture to picture;
 *             picture_structure 3 and frame_pred_frame_dct 1 are required
 *   sequence  load_intra_quantiser_matrix / load_non_intra_quantiser_matrix: 64 bytes each, zig-zag order, 0 forbidden
 *   macroblock  macroblock_address_increment (Table B-1) with macroblock_escape; skipped macroblocks in P pictures (7.6.6); all of
 *             Tables B-2 and B-3; a macroblock's quantiser_scale_code replaces the slice's (0 is refused)
 * Still M2V_DEC_SYNTAX in the main syntax, the follow-ups: leading B pictures (fewer than two anchors in front of them) and D pictures;
 * field pictures; every scalable extension; size extensions and sizes over 2048; chroma formats other than 4:2:0; a skipped macroblock in an I picture;
 * an increment that passes the row's end; vectors that read outside the picture; and every check the module syntax makes on codes,
 * coefficient indices and stuffing inside a slice.  Refused unless their option is on (each below): B pictures ("decode_b_pictures");
 * frame_pred_frame_dct 0 ("decode_interlaced"); more than one slice in a macroblock row, a slice whose first increment is not 1 or
 * whose row ends short, a slice header with intra_slice_flag 1, quant_matrix_extension and composite_display_flag 1 (without the option
 * its 20 bits are read as stuffing that is not zero) ("decode_extended"); intra_vlc_format 1 (Table B-15), concealment_motion_vectors 1
 * and dual prime ("decode_mb_tools" on top of "decode_extended").  The batch entry for the main syntax is
 * m2v_decode_streams_main_device, below.
 *
 * Option "decode_b_pictures" (m2v_set_option), per handle: 0 (the default) - everything above, bit for bit, launch for launch and
 * refusal for refusal (a B picture is M2V_DEC_SYNTAX at its picture header); 1 - B pictures are decoded too, and the frames come out
 * in DISPLAY order.  Any other value is M2V_E_PARAM.  With 1, "decode_syntax" must be M2V_SYNTAX_MAIN and `mode` M2V_DEC_ISO:
 * otherwise m2v_decode_device returns M2V_E_PARAM, writes nothing and m2v_last_error names the option; m2v_decode_streams_device is
 * what it was.  The definition is decoder.decode(stream, quirks=False, syntax="main", b_pictures=True); every stream the main syntax
 * accepts with the option off decodes, with it on, to the same bytes and the same record.  Added to what the main syntax accepts:
 *   picture   picture_coding_type 3, with full_pel_backward_vector 0 and backward_f_code (not judged) in the picture header and all four
 *             f_codes 1 .. 9 in its coding extension.  An anchor is an I or P picture; a P picture predicts from the last anchor in
 *             front of it in coded order, a B picture forward from the anchor before the last and backward from the last, whatever GOP
 *             headers lie between (temporal_reference, closed_gop and broken_link are read and ignored)
 *   macroblock  Table B-4; two vector predictors, both reset at the start of a slice and behind an intra macroblock, each kept by a
 *             macroblock that does not use its direction; forward vectors with f_code[0][t], backward with f_code[1][t]; both
 *             directions: each prediction rounded on its own, then (a + b + 1) >> 1; a skipped macroblock takes the directions and
 *             vectors of the macroblock in front of it (refused behind an intra macroblock); a vector of either direction that reads
 *             outside the picture refuses the slice, a skipped macroblock's included
 *   order     display order from coded order and picture types alone: a B picture is put out when decoded, an anchor when the next
 *             anchor arrives or at the end - coded picture p lies at display index p - 1 if it is a B picture, else at (coded index
 *             of the next anchor) - 1, the last anchor at pictures - 1.  The picture with display index d lies at d * frame_bytes, in
 *             every layout; a stream without B pictures has display = coded
 * The record, err_offset, probe calls, M2V_DEC_OVERFLOW, "decode_batch" (the result does not depend on it) and the container path are
 * unchanged; pictures of chunks in front of the one in which a slice is refused may have been written, at their display indices.
 *
 * Option "decode_interlaced" (m2v_set_option), per handle: 0 (the default) - everything above, bit for bit, launch for launch and
 * refusal for refusal (frame_pred_frame_dct 0 is M2V_DEC_SYNTAX at its picture coding extension); 1 - interlaced FRAME pictures are
 * decoded too: field prediction and field DCT.  Any other value is M2V_E_PARAM.  With 1, "decode_syntax" must be M2V_SYNTAX_MAIN and
 * `mode` M2V_DEC_ISO: otherwise m2v_decode_device returns M2V_E_PARAM, writes nothing and m2v_last_error names the option;
 * m2v_decode_streams_device is what it was.  It combines with "decode_b_pictures" 0 (a B picture is still refused at its picture
 * header, frames in coded order) or 1 (frames in display order, as above).  The definition is decoder.decode(stream, quirks=False,
 * syntax="main", b_pictures=..., interlaced=True).  Every stream the main syntax accepts with the option off - "decode_b_pictures"
 * either way - decodes, with it on, to the same bytes and the same record, with ONE exception: a stream with progressive_sequence 0
 * whose (height + 15) / 16 is odd has one more macroblock row with the option on (first line below) and is another stream.  Added:
 *   sequence  with progressive_sequence 0 a picture has 2 * ((height + 31) / 32) macroblock rows (6.3.3): slice codes run to that, the
 *             coded picture is 16 times that many lines, cropped to the header's size as always (16 lines: two slices a picture).
 *             With progressive_sequence 1 nothing changes
 *   picture   frame_pred_frame_dct 0 where progressive_sequence and progressive_frame are both 0; refused at the extension where either
 *             is 1 (6.3.10).  top_field_first, repeat_first_field and chroma_420_type are read and not acted on: one coded picture is
 *             one output frame with both fields woven, whatever repeat_first_field says.  picture_structure stays 3; a picture
 *             with frame_pred_frame_dct 1 decodes exactly as without the option
 *   modes     in a picture with frame_pred_frame_dct 0: frame_motion_type (2 bits) behind macroblock_type where the macroblock has a
 *             forward or backward vector, then dct_type (1 bit) where it is intra or has a pattern, then quantiser_scale_code and the
 *             rest.  frame_motion_type 2 is frame-based, 1 field-based; 0 (reserved) and 3 (dual prime) refuse the slice
 *   vectors   two predictors per direction, PMV[r][s].  A field-based macroblock carries, per direction it uses, field select and
 *             vector for its top-field lines, then for its bottom-field lines; vector r from PMV[r][s], its vertical component from
 *             PMV[r][s][1] >> 1 with the unchanged delta, wrap and range of f_code[s][1], and PMV[r][s][1] = 2 * vector afterwards.  A
 *             frame vector is predicted from PMV[0][s] and sets PMV[1][s] to it.  All are reset at a slice's start, behind an intra
 *             macroblock, behind a P picture's macroblock without a vector and behind a P picture's skipped macroblock
 *   prediction  field-based (7.6.4): vector 0 predicts the macroblock's frame rows 0, 2 .. 14, vector 1 its rows 1, 3 .. 15, each from
 *             the field of the reference its select names (0: the even rows), in half samples of that field: field line
 *             8 * row + j + (vy >> 1), with vy & 1 the rounded mean with the next line of the same field; horizontally as ever.
 *             Chroma: both components / 2 toward zero, four lines per field.  Both directions: each formed in full, then
 *             (a + b + 1) >> 1.  A field vector that reads outside its field (16 x 8 luma at (16 col, 8 row) of 16 mbw x 8 mbh; chroma
 *             8 x 4 with the halved vector) refuses the slice
 *   dct_type 1  luma blocks 0 / 1 are the macroblock's top-field lines (row k of the block is row 2k), 2 / 3 its bottom-field lines
 *             (row 2k + 1); chroma blocks are frame blocks; inverse quantisation, mismatch control and the IDCT are untouched
 *   skipped   frame prediction: a P picture's with the zero vector; a B picture's in the directions of the macroblock in front with
 *             PMV[0][s] read as frame vectors - behind a field-based macroblock twice its first field vector's vertical component
 * Still M2V_DEC_SYNTAX with the option on: field pictures (picture_structure 1 and 2: option "decode_field_pictures" below); dual prime and concealment vectors (option
 * "decode_mb_tools" below reads them); and everything else the main syntax refuses.
 *
 * Option "decode_extended" (m2v_set_option), per handle: 0 (the default) - everything above, bit for bit, launch for launch and
 * refusal for refusal; 1 - several slices in a macroblock row, slice headers with intra_slice_flag 1, quant_matrix_extension and
 * composite_display_flag 1 are read too.  Any other value is M2V_E_PARAM.  With 1, "decode_syntax" must be M2V_SYNTAX_MAIN and `mode`
 * M2V_DEC_ISO: otherwise m2v_decode_device returns M2V_E_PARAM, writes nothing and m2v_last_error names the option;
 * m2v_decode_streams_device is what it was.  It combines with "decode_b_pictures" and "decode_interlaced" in all four settings.  The
 * definition is decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=..., extended=True).  Every stream the
 * main syntax accepts with the option off, under any setting of the other two, decodes with it on to the same bytes and the same
 * record.  Added (6.2.4, 6.3.16: the restricted slice structure Main Profile requires; 6.2.3.2, 6.3.11):
 *   slices    a picture is any number of slices, 1 <= slice code <= the macroblock rows (as the other options define them).  The
 *             grammar stays local: the first slice behind a picture's extensions has code 1, every further one its predecessor's
 *             code or that code + 1, and a picture may end only behind a slice with the last row's code.  A slice's first
 *             macroblock_address_increment, escapes included, gives its first column as increment - 1; nothing is skipped in front
 *             of it.  The macroblock loop runs until nothing but zero bits is left in the unit (the standard's test of 23 zero bits
 *             gives the same verdict: 23 zero bits begin no macroblock).  A slice without a macroblock is refused, and one whose
 *             column passes the row's last.  DC predictors and all vector predictors reset at every slice start; skipped
 *             macroblocks inside a slice are what each picture type defines above
 *   continuity  judged behind the walk: the first slice of a row starts at column 0 and the row in front of it is full; a slice with
 *             its predecessor's code starts at the predecessor's last column + 1; the picture's last slice ends at the row's last
 *             column.  A slice that breaks one of these is refused at its own start code.  err_offset stays the earliest unit the
 *             grammar refuses, else the earliest slice in error - one that cannot be read or one that breaks continuity (a slice behind
 *             an unreadable one is not judged: the unreadable one is earlier).  Nothing of a chunk with such a slice is written
 *   header    behind quantiser_scale_code a bit 1 is intra_slice_flag: intra_slice (1 bit) and reserved_bits (7 bits) follow, read
 *             and not judged; then, while the next bit is 1, extra_bit_slice and extra_information_slice (8 bits, skipped); then the
 *             closing 0.  With intra_slice_flag 0 the header is as above
 *   matrices  quant_matrix_extension (identifier 3) among the units that may follow a picture_coding_extension, in any order with
 *             user_data, copyright_extension and picture_display_extension; one a picture at most (a second is refused at the
 *             second), anywhere else refused at its start code.  load_intra_quantiser_matrix and load_non_intra_quantiser_matrix
 *             with 64 bytes each in zig-zag order (a weight of 0 refuses the unit), the two chroma load flags 0 (4:2:0 only), zero
 *             stuffing.  A loaded matrix is in force from that picture on in CODED order, each matrix on its own; any sequence header,
 *             repeated ones included, puts both back to the sequence's
 *   composite  composite_display_flag 1: the 20 bits behind it are read and not acted on
 * Out of scope, the follow-ups: m2v_decode_streams_main_device keeps its two flags (any other bit stays M2V_E_PARAM); field pictures
 * (without option "decode_field_pictures"), leading B pictures and D pictures stay refused, dual prime, concealment vectors and Table B-15 too without option "decode_mb_tools",
 * and everything else the main syntax refuses stays refused where it is refused without the option.
 *
 * Option "decode_mb_tools" (m2v_set_option), per handle: 0 (the default) - everything above, bit for bit, launch for launch and
 * refusal for refusal; 1 - the rest of the macroblock layer of frame pictures is read too.  Any other value is M2V_E_PARAM.  With 1,
 * "decode_syntax" must be M2V_SYNTAX_MAIN, `mode` M2V_DEC_ISO and "decode_extended" 1 (its slice walk is the one that reads every
 * picture kind in one function, and its grammar is a superset: no stream is lost): otherwise m2v_decode_device returns M2V_E_PARAM,
 * writes nothing and m2v_last_error names the option.  It combines with "decode_b_pictures" and "decode_interlaced" in all four
 * settings.  The definition is decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=..., extended=True,
 * mb_tools=True).  Every stream accepted with the option off decodes with it on to the same bytes and the same record; a stream it
 * refuses is M2V_DEC_SYNTAX with the offset of the unit in error.  Added (6.3.10, 6.3.17.2, 7.2.2, 7.6.3.6, 7.6.3.9, Table B-15):
 *   Table B-15  with a picture's intra_vlc_format 1 the AC coefficients of INTRA blocks are read with Table B-15 (end of block '0110',
 *             escape '000001' with the same body); non-intra blocks keep Table B-14 and its '1s' first-coefficient form; DC sizes, the
 *             scans and everything behind the level are unchanged.  A B-14 codeword that Table B-15 does not hold refuses the slice
 *   concealment  with concealment_motion_vectors 1 an intra macroblock carries, behind its quantiser and in front of its blocks, one
 *             forward frame vector (motion_code and residual, horizontal then vertical, f_code[0][*]; no frame_motion_type, no field
 *             select) and a marker_bit that must be 1.  The vector sets PMV[0][0] and PMV[1][0]; it is not used in reconstruction
 *             and not judged against the picture's edges; such a macroblock does not reset the vector predictors (one without
 *             concealment vectors still does).  In an I picture with the flag f_code[0][0] and f_code[0][1] must be 1 .. 9
 *   dual prime  frame_motion_type 3 in a P picture with frame_pred_frame_dct 0 ("decode_interlaced" on); in a B picture it stays
 *             refused, and whether B pictures lie between the picture and its reference is not judged.  One vector without a field
 *             select: motion_code[0][0][0], dmvector[0], motion_code[0][0][1], dmvector[1] (dmvector '0' 0, '10' +1, '11' -1); the
 *             vertical component is a field vector, predicted from PMV[0][0][1] >> 1, the predictor twice the vector afterwards,
 *             PMV[1][0] = PMV[0][0].  With h(a) = (a + (a > 0)) >> 1 and top_field_first 1, T = (h(vx) + d0, h(vy) + d1 - 1) and
 *             B = (h(3 vx) + d0, h(3 vy) + d1 + 1); with top_field_first 0 the factors 1 and 3 change places.  Top-field lines are
 *             the mean (a + b + 1) >> 1 of the reference's top field by (vx, vy) and its bottom field by T, bottom-field lines of
 *             its bottom field by (vx, vy) and its top field by B; each a 16 x 8 field prediction with half-sample interpolation,
 *             each vector halved toward zero on its own for chroma.  All four reads must lie inside their field, or the slice is
 *             refused.  A skipped macroblock behind a dual-prime one is the zero vector, as ever
 * Still M2V_DEC_SYNTAX: leading B pictures, D pictures - field pictures too without option "decode_field_pictures", below.
 * m2v_decode_streams_main_device takes neither "decode_extended" nor "decode_mb_tools"; the batch entry that does is
 * m2v_decode_streams_main_ex_device, below.
 *
 * Option "decode_field_pictures" (m2v_set_option), per handle: 0 (the default) - everything above, bit for bit, launch for launch and
 * refusal for refusal; 1 - field pictures are read too.  Any other value is M2V_E_PARAM.  With 1, "decode_syntax" must be
 * M2V_SYNTAX_MAIN, `mode` M2V_DEC_ISO and "decode_interlaced", "decode_extended" and "decode_mb_tools" all 1 (that grammar is a
 * superset - no stream is lost - and field pictures need its selects, dual prime and concealment vectors): otherwise
 * m2v_decode_device returns M2V_E_PARAM, writes nothing and m2v_last_error names the option.  "decode_b_pictures" may be 0 or 1.  The
 * definition is decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=True, extended=True, mb_tools=True,
 * field_pictures=True).  Every stream accepted with the option off decodes with it on to the same bytes and the same record.  Added
 * (6.1.1.4, 6.3.10, 6.3.17, 7.6.2 - 7.6.3.6, 7.6.6, 7.6.7):
 *   extension  picture_structure 1 (top field) and 2 (bottom field) where progressive_sequence, progressive_frame,
 *             frame_pred_frame_dct, top_field_first and repeat_first_field are all 0; value 0 is refused; all at the coding extension
 *   pairs      a coded frame is one frame picture or two field pictures that follow each other in coded order: opposite parity in
 *             either order, the same temporal_reference, the same picture_coding_type or a P field behind an I field.  A picture
 *             behind a first field that is not such a partner - the same parity, a frame picture, another type, another
 *             temporal_reference - is refused at its picture header; a sequence header, a GOP header or sequence_end_code between the
 *             two fields at its start code (the second field's header, extensions, user_data and the transparent units may stand
 *             there); a first field no picture follows at its own picture header.  Frame pictures and field pairs may be mixed
 *   geometry   a field has (height + 31) / 32 macroblock rows, its slice codes run to that, continuity is judged per field; row r,
 *             line k of the field of parity p is frame line 32 r + 2 k + p; the frame is cropped to the header's size as ever
 *   modes      field_motion_type (2 bits) where the macroblock has a vector: 1 field-based (one vector a direction), 2 16 x 8 (two),
 *             3 dual prime (a P field only), 0 refused; no dct_type.  motion_vertical_field_select in front of every vector of the
 *             first two kinds.  No component is halved going in or doubled coming out.  Field-based: predicted from PMV[0][s],
 *             PMV[1][s] = PMV[0][s] afterwards; 16 x 8: vector r from and into PMV[r][s]; dual prime: no select, dmvector behind each
 *             component, PMV[1][0] = PMV[0][0].  A concealment vector carries a select (read, not used) and its marker bit
 *   prediction the field a select names is the most recently decoded anchor field of that parity: the two fields of the anchor
 *             frame(s) - but for the second field of an anchor frame the field of the other parity is the first field of its own
 *             frame.  A select that names a field that does not exist (the field's own parity in the second field of the stream's first
 *             frame) refuses the slice.  Field-based 16 x 16 (chroma 8 x 8); 16 x 8: the upper half by vector 0, the lower by vector
 *             1 (chroma 8 x 4 each); dual prime: (a + b + 1) >> 1 of the same parity by (vx, vy) and the other parity by
 *             (h(vx) + d0, h(vy) + d1 + e), e = -1 in a top field, + 1 in a bottom field.  Every read inside its field.  A P field's
 *             macroblock without a vector and its skipped macroblock: the zero vector, its own parity, the predictors reset; a B
 *             field's skipped macroblock: the directions in front, the predictors as vectors, field-based, its own parity
 *   record     one output frame a coded frame, both fields woven; a frame's type is its first field's (I + P is an I frame);
 *             pictures, gops, chains and repeated_headers count FRAMES, out_bytes = pictures * frame_bytes, "decode_batch" counts
 *             frames (a chunk's edge never parts a pair).  A B pair needs two anchor frames in front of it
 * Out of scope, the follow-ups: m2v_decode_streams_main_ex_device keeps its four flags (bit 16 stays M2V_E_PARAM); leading B pictures
 * and D pictures stay refused (leading B pictures: option "decode_join", below); repeat_first_field and display timing.
 *
 * Option "decode_join" (m2v_set_option), per handle: a mask of M2V_JOIN_HEAD (1) and M2V_JOIN_TAIL (2), 0 .. 3; any other value is
 * M2V_E_PARAM.  0 (the default) - everything above, bit for bit, launch for launch and refusal for refusal.  For a stream cut from a
 * running broadcast: it begins wherever the recording began, its first B pictures refer to an anchor that is not there, and it breaks
 * off inside a picture.  With a value other than 0, "decode_syntax" must be M2V_SYNTAX_MAIN, `mode` M2V_DEC_ISO and
 * "decode_interlaced", "decode_extended", "decode_mb_tools" and "decode_field_pictures" all 1 (the superset once more: one plan learns
 * this, not six): otherwise m2v_decode_device returns M2V_E_PARAM, writes nothing and m2v_last_error names the option.
 * "decode_b_pictures" may be 0 or 1.  The batch entries neither read nor change the option.  The definition is
 * decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=True, extended=True, mb_tools=True,
 * field_pictures=True, join=1 .. 3).  Every stream accepted with the option off decodes with bit 1 on to the same bytes and the same
 * record; with bit 2 on that holds for the streams that end with sequence_end_code - a complete stream without one loses its last
 * frame (below), which is why the tail is a bit of its own: a file a tool cut at a GOP wants bit 1 alone.
 *   head (1)   J is the offset of the first sequence_header_code the start-code scan finds.  Bytes and start codes in front of J are
 *             not read any further and not judged; without one the stream is refused at offset 0.  The header group at J is "the
 *             first sequence header" of every rule above - its size rules, the macroblock rows, what repeated headers must equal -
 *             and a wrong one is refused at its own unit: no later one is looked for.  err_offset stays relative to the first byte of
 *             the input, es_bytes is the whole input.
 *             Leading B pictures (with "decode_b_pictures" 1; with 0 a B picture is refused at its header as ever): a B picture that
 *             begins a frame while fewer than two anchor FRAMES have begun since J is dropped where it was refused, a B field pair
 *             as a pair.  A dropped picture's units are judged by the grammar exactly as a kept picture's - header, coding
 *             extension, the rules of a pair, slice codes, one quant_matrix_extension at most -, and a matrix it loads holds from that
 *             picture on; its slices are not walked (no slice refusal, no continuity verdict).  It has no frame index, no display
 *             index and no room in the output and is not counted in `pictures`: display indices are those of the kept frames.  A P
 *             picture with no I frame in front of it since J stays refused at its header.
 *   tail (2)   where the last significant unit is sequence_end_code nothing is dropped.  Otherwise F is the last picture start code
 *             that begins a frame - pairs as above: the picture behind a waiting first field is its partner, whatever it is; a picture
 *             start code whose header does not read begins a frame unless a first field waits -, and T the offset of the first group_start_code or
 *             picture_start_code behind the last slice in front of F (behind the first unit read where there is no such slice).  The
 *             stream is read as its bytes [J, T) (J = 0 without bit 1), exactly as a stream that ends at T; the units from T on are
 *             not judged.  One frame counts as dropped.  A frame is known by its picture start code alone: while the bytes behind the
 *             last whole frame hold none yet - fewer than four bytes of it, or a sequence or GOP header alone - F is that last whole
 *             frame, and it goes.  The rule is blunt on purpose: the last picture of a recording is cut at an
 *             arbitrary byte, and a cut inside its last row could only be found by the slice walk, after the layout is fixed.
 *   A stream in which no frame is left is a stream without pictures: M2V_DEC_OK, pictures 0.
 * m2v_decode_join_report describes the same call as m2v_decode_report: join_offset = J, tail_offset = T (es_bytes where nothing was
 * dropped behind), the dropped FRAMES in front and behind (dropped_trailing is 0 or 1).  It answers 0, es_bytes, 0, 0 for a call with
 * the option off and for a refused stream.  A caller who records in segments keeps the bytes [tail_offset, es_bytes) for the front of
 * the next segment.  m2v_decode_stat is what it was, `reserved` 0.
 * Out of scope: the batch entries; resynchronising behind damage in the middle of a stream; a sequence header that changes
 * mid-stream; D pictures; repeat_first_field and display timing; the module syntax.
 *
 * Option "decode_conceal" (m2v_set_option), per handle: 0 (the default) or 1; any other value is M2V_E_PARAM.  0 - everything above,
 * bit for bit, launch for launch and refusal for refusal.  1 - a damaged slice no longer refuses the stream: the slice is dropped, the
 * hole is patched from the frame in front, and the call answers M2V_DEC_OK with the record of the undamaged stream.  It has the
 * requirements of "decode_join": "decode_syntax" M2V_SYNTAX_MAIN, `mode` M2V_DEC_ISO and "decode_interlaced", "decode_extended",
 * "decode_mb_tools" and "decode_field_pictures" all 1; otherwise m2v_decode_device returns M2V_E_PARAM, writes nothing and
 * m2v_last_error names the option.  "decode_b_pictures" may be 0 or 1, "decode_join" 0 .. 3.  The batch entries neither read nor
 * change the option.  The definition is decoder.decode(stream, ..., field_pictures=True, join=..., conceal=True).  Every stream accepted
 * with the option off decodes with it on to the same bytes and the same record, and a report of zeros.
 *   grammar    a slice is legal behind a picture coding extension or behind a slice, whatever the two codes are.  A slice whose code
 *             is above the picture's macroblock rows (a field's rows for a field) is a BAD SLICE: counted, not walked, not refused.  A
 *             sequence header, GOP header, picture header or sequence_end_code, and the end of the stream, are legal behind a slice of
 *             any code or behind a picture coding extension (a picture with no slice left).  Everything else is judged as with the
 *             option off - headers, extensions, the pairing of fields, "P without an I frame", "B without two anchor frames", a second
 *             quant_matrix_extension, the join window -, and a stream refused there is M2V_DEC_SYNTAX at the same offset: damage to
 *             a header stays a refusal
 *   rows       the unit of concealment is the macroblock row of a coded picture (a field's row for a field).  A row is KEPT if and
 *             only if the slices of its picture that carry its code, in stream order, all read, the first starts at column 0, each
 *             further one starts one column behind the last column of the one in front, and the last ends at column mbw - 1.  Any
 *             other row is CONCEALED whole: one with no slice, with a slice that does not read (a bad slice too), with a gap, an
 *             overlap or a duplicate.  The rule is blunt on purpose: where inside a slice an error is noticed is not pinned, only the
 *             verdict per slice is; and whatever a damaged slice's walk left in its row - it writes nowhere else - is overwritten
 *   patch      every macroblock of a concealed row of a frame picture is a P picture's skipped macroblock: forward, frame-based,
 *             vector (0, 0), no residual; of a field picture: forward, field-based from the field of its own parity, vector (0, 0).  The
 *             reference is the frame the picture's forward reference names: for P the anchor frame in front, for B the earlier of its
 *             two, for an I picture the anchor frame in front as if it were P; a second field takes its own parity from that frame
 *             too, never from its own.  Where there is no such frame (the first anchor frame of the stream or of the join window,
 *             both of its fields) the macroblock is intra without a block: Y = U = V = 128, a GREY ROW.  A concealed picture is a
 *             reference like any other
 * m2v_decode_conceal_report describes the same call as m2v_decode_report: first_offset is the offset, from the first byte of the
 * input, of the picture start code of the first coded picture in coded order with a concealed row (es_bytes where there is none);
 * bad_slices, concealed_rows, grey_rows count what their names say, damaged_pictures coded pictures with a concealed row.  The counts
 * are summed on the device and come with the record: no further wait.  They do not depend on "decode_batch".  All zero (first_offset
 * es_bytes) for a call with the option off and for a call that did not answer M2V_DEC_OK.
 * Out of scope: damage to any header; keeping the macroblocks in front of an error; motion-compensated or spatial concealment;
 * transport_error_indicator and continuity faults from the demultiplexer; the batch entries; D pictures; repeat_first_field.
 */
enum { M2V_DEC_ISO = 0, M2V_DEC_MODULE = 1 };
enum { M2V_SYNTAX_MODULE = 0, M2V_SYNTAX_MAIN = 1 };                            /* option "decode_syntax" */
enum { M2V_DEC_OK = 0, M2V_DEC_SYNTAX = -2, M2V_DEC_OVERFLOW = -3 };
typedef struct { uint64_t es_bytes, out_bytes, frame_bytes, err_offset;
                 uint32_t pictures, gops, width, height, repeated_headers, chains;
                 int32_t status; uint32_t reserved[3]; } m2v_decode_stat;      /* 72 bytes */
int m2v_decode_device(m2v_enc *e, const void *d_es, size_t es_bytes, void *d_dst, size_t cap, int layout, int mode, void *hip_stream);
int m2v_decode_report(m2v_enc *e, m2v_decode_stat *out);
enum { M2V_JOIN_HEAD = 1, M2V_JOIN_TAIL = 2 };                                  /* option "decode_join" */
typedef struct { uint64_t join_offset, tail_offset; uint32_t dropped_leading, dropped_trailing, reserved[2]; } m2v_decode_join;   /* 32 bytes */
int m2v_decode_join_report(m2v_enc *e, m2v_decode_join *out);
typedef struct { uint64_t first_offset; uint32_t bad_slices, concealed_rows, grey_rows, damaged_pictures, reserved[2]; } m2v_decode_conceal;   /* 32 bytes */
int m2v_decode_conceal_report(m2v_enc *e, m2v_decode_conceal *out);
int m2v_decode_scan_tile(void);

/*
 * Several streams per call: m2v_decode_streams_device decodes a batch of elementary streams of ANY picture sizes in one call, each judged
 * alone, the frames packed one stream behind the other.  ("streams", not "batch": option "decode_batch" means pictures per chunk.)
 *
 * Segments.  nstreams is 1 .. 65535 (anything else: M2V_E_PARAM).  Stream b is the es_bytes[b] bytes at d_es + es_off[b], at any byte
 * address; segments may touch or leave gaps.  Nothing outside a segment is read or interpreted: a start code in a gap, or one that
 * straddles a segment's edge, does not exist.  layout and mode are the call's, as in m2v_decode_device.
 *
 * Each stream is judged alone.  `rec` is field for field what m2v_decode_device reports for that stream decoded by itself, err_offset
 * relative to the stream's first byte; decoder.py stays the specification.  One stream's M2V_DEC_SYNTAX changes nothing about any other
 * stream's frames or record.  A segment of fewer than 4 bytes is M2V_DEC_SYNTAX.  Streams of one call may have different picture sizes
 * (the rendition ladder of m2v_set_source_size is the obvious batch).
 *
 * Layout of the output.  Frames are packed with no rounding between streams: stream b's picture n is at out_offset[b] + n * frame_bytes[b],
 * and out_offset[b] is the sum of pictures * frame_bytes over the streams in front of it that the PROBE STAGE accepts - the headers and
 * the grammar of the start codes: exactly what a call with d_dst == NULL finds.  A probe call (d_dst == NULL) reports out_offset and
 * out_bytes per stream, and a decode has exactly the layout its probe reports, whatever cap is.  A stream refused at the probe stage takes
 * no room (its out_offset is where it would have stood).  A stream refused inside a slice is found after the layout is fixed: it keeps
 * its room, reports out_bytes 0, and not one byte of that room is written.  A stream whose room does not lie wholly inside cap is
 * M2V_DEC_OVERFLOW, with nothing written; the others are written.  Nothing outside the rooms of OK streams is ever written.  With all
 * streams OK and equal in size and length the output is a [B, N, frame_bytes] tensor, the mirror of encode_batch's input.
 *
 * The call blocks and answers M2V_OK once the kernels ran; the verdicts are in the records, which m2v_decode_streams_report pops, oldest
 * first (out NULL: how many wait) and which are dropped at the next m2v_decode_streams_device.  M2V_E_STATE while a sequence is in
 * progress or a resident call is in flight.  There are TWO host waits per call whatever nstreams is: one behind the plan - sizes, picture
 * types, the layout - and one at the end (a third when a stream holds more start codes than its list was guessed to: the scan then runs
 * again with the counts of the first run, as in m2v_decode_device).  An error the slice walk finds stays on the device.
 *
 * Chunks.  A chunk is a run of whole pictures in batch order; it may cut a stream between an I and a P picture, or end at a stream
 * boundary.  Option "decode_batch", when set, is pictures per chunk, as before.  When it is 0 THIS entry's default is the 256 MiB bound on
 * the chunk's levels alone, counted from each picture's own macroblocks (768 bytes each): there is no 256-picture ceiling here, because
 * the batch of small clips - 64 clips x 9 pictures of 320 x 240 are one chunk - is the case this entry exists for.  The result does not
 * depend on the chunks.  The slices of a stream that lies in more than one chunk are walked twice: once in front of all chunks for the
 * verdict alone, so that a stream refused in a late slice has none of its early pictures written.
 *
 * m2v_decode_device is unchanged, and its kernels are its own: this entry runs kernels of its own over the same arithmetic.
 */
typedef struct { uint64_t es_offset, out_offset; m2v_decode_stat rec; } m2v_decode_stream_stat;   /* 88 bytes */
int m2v_decode_streams_device(m2v_enc *e, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams,
                              void *d_dst, size_t cap, int layout, int mode, void *hip_stream);
int m2v_decode_streams_report(m2v_enc *e, m2v_decode_stream_stat *out, size_t max);   /* pops, oldest first; out NULL: how many wait */

/*
 * The batch entry of the MAIN syntax: m2v_decode_streams_main_device decodes a batch of main-syntax elementary streams - what
 * m2v_demux_device extracts from an ordinary multiplexer's containers - in one call.  m2v_decode_streams_device does not move: it reads
 * the module's dialect and still answers M2V_E_STATE while "decode_syntax" is main.
 *
 * The syntax is the CALL's, not the handle's: the entry neither reads nor changes "decode_syntax", "decode_b_pictures" or
 * "decode_interlaced".  flags: M2V_DECS_B_PICTURES (1) accepts B pictures, M2V_DECS_INTERLACED (2) accepts frame pictures with
 * frame_pred_frame_dct 0; any other bit is M2V_E_PARAM, m2v_last_error names the entry, nothing is touched.  The mode is M2V_DEC_ISO (the
 * module's quirks have no meaning here).  It does read "decode_batch", as the module's entry does.
 *
 * Segments, nstreams 1 .. 65535, d_dst == NULL as a probe call, cap, layout, blocking, the two host waits per call (a third when a
 * stream holds more start codes than guessed) and M2V_E_STATE while a sequence is in progress or a resident call is in flight are word
 * for word m2v_decode_streams_device's contract, above.  The records are m2v_decode_stream_stat, popped through
 * m2v_decode_streams_report: the same queue, dropped at the next call of EITHER batch entry.
 *
 * Each stream is judged alone.  `rec` is field for field what m2v_decode_device reports for that stream by itself with "decode_syntax" =
 * main, "decode_b_pictures" = (flags & 1) and "decode_interlaced" = (flags >> 1 & 1): decoder.decode(stream, quirks=False,
 * syntax="main", b_pictures=, interlaced=) is the definition, rec.err_offset is Refused.offset relative to the stream's first byte.
 *
 * Layout.  The rules are the module entry's: out_offset[b] sums pictures * frame_bytes over the streams in front that the probe stage
 * accepts - the headers and the grammar of the start codes (decoder._main_plan does not raise).  A stream refused there takes no room.
 * With flag 1 off a B picture is such a refusal at its picture header, with flag 2 off frame_pred_frame_dct 0 is one at its coding
 * extension: the same batch has different layouts under different flags.  A stream refused inside a slice keeps its room and not one byte
 * of it is written, in however many chunks it lies; a stream whose room does not lie inside cap is M2V_DEC_OVERFLOW; nothing outside
 * the rooms of OK streams is ever written.
 *
 * Frame order.  With flag 1 on, a stream's frames are in DISPLAY order inside its room: coded picture p lies at out_offset +
 * display[p] * frame_bytes, `display` as the B-picture paragraph above defines it.  With flag 1 off they are in coded order (the same
 * thing: there is no B picture).  With flag 2 on a progressive_sequence 0 stream has 2 * ((height + 31) / 32) macroblock rows, the same
 * stated exception as in the single-stream option.  The result does not depend on "decode_batch": a stream cut at a chunk's edge
 * carries its last two anchors into the next chunk.
 *
 * Still M2V_DEC_SYNTAX, exactly where the single-stream decoder refuses them: intra_vlc_format 1 (Table B-15), quant_matrix_extension,
 * several slices in a macroblock row, intra_slice_flag, field pictures, dual prime, concealment vectors.
 */
enum { M2V_DECS_B_PICTURES = 1, M2V_DECS_INTERLACED = 2 };
int m2v_decode_streams_main_device(m2v_enc *e, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams,
                                   void *d_dst, size_t cap, int layout, unsigned flags, void *hip_stream);

/*
 * The batch entry of the main syntax WITH the extended options: m2v_decode_streams_main_ex_device is m2v_decode_streams_main_device with
 * two further flags.  M2V_DECS_EXTENDED (4) is what "decode_extended" is to m2v_decode_device: several slices in a macroblock row,
 * intra_slice_flag with its extras, quant_matrix_extension, composite_display_flag 1.  M2V_DECS_MB_TOOLS (8) is "decode_mb_tools":
 * Table B-15, concealment motion vectors, dual prime.  m2v_decode_streams_main_device keeps its two flags and its kernels.
 *
 * The contract is m2v_decode_streams_main_device's, word for word: segments at any byte address, nstreams 1 .. 65535, d_dst == NULL as a
 * probe call, cap, the packed layout with out_offset, display order with flag 1, blocking, two host waits per call (a third when a stream
 * holds more start codes than guessed), M2V_E_STATE in the same situations, "decode_batch" read, the mode M2V_DEC_ISO.  The records are
 * popped through the same m2v_decode_streams_report queue; a call of any of the three batch entries drops that queue.  None of the five
 * decode_* options of the handle is read or changed.
 *
 * flags.  Any bit above 8 is M2V_E_PARAM, and so is M2V_DECS_MB_TOOLS without M2V_DECS_EXTENDED (the single-stream rule);
 * m2v_last_error names the entry, nothing is touched.  With flags < 4 the entry runs m2v_decode_streams_main_device's implementation:
 * the same bytes, the same records, the same launches.
 *
 * Each stream is judged alone.  `rec` is what m2v_decode_device reports for it with the four options set as the flags say:
 * decoder.decode(stream, quirks=False, syntax="main", b_pictures=f & 1, interlaced=f & 2, extended=f & 4, mb_tools=f & 8) is the
 * definition.  A refusal is at the probe stage - the stream takes no room - iff decoder._main_plan(stream, b, i, x, t) raises: so Table
 * B-15, concealment vectors or dual prime's intra_vlc_format / concealment_motion_vectors under flags 4 .. 7 are a probe refusal at the
 * picture coding extension, and the same batch has different layouts under different flags.  Every other refusal is at the slice stage,
 * also that of a slice which breaks the continuity of its row or its picture (refused at its own start code): the stream keeps its
 * room and not one byte of it is written, in however many chunks it lies.  M2V_DEC_OVERFLOW, and "nothing outside the rooms of OK
 * streams is ever written", hold as before.  The result does not depend on "decode_batch": a quant_matrix_extension stays in force
 * across chunks until a sequence header puts the sequence's matrices back, and a dual-prime P picture that is the first anchor of its
 * chunk reads both predictions from the carried slot.
 *
 * Still M2V_DEC_SYNTAX, as in the single-stream decoder: field pictures, leading B pictures, D pictures.
 */
enum { M2V_DECS_EXTENDED = 4, M2V_DECS_MB_TOOLS = 8 };
int m2v_decode_streams_main_ex_device(m2v_enc *e, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams,
                                      void *d_dst, size_t cap, int layout, unsigned flags, void *hip_stream);

/*
 * Demux on the device: the inverse of m2v_mux_device.  nstreams (1 .. 65535) transport (kind M2V_MUX_TS) or program (M2V_MUX_PS) streams
 * in device memory - container i is the src_bytes[i] bytes at d_src + src_off[i], at ANY byte address - back to the video elementary
 * stream of each, which m2v_decode_device takes.  `stream`: the PID (0 .. 0x1FFF) / stream_id (0xE0 .. 0xEF) to take in every container,
 * or -1: found in each (PAT and PMT; the first video packet of the chain).  The bytes, the stamps and every field of a record are what
 * m2vc_demux_ts / m2vc_demux_ps (include/m2v_container.h: the specification, with every rule) answer for that container, with the
 * stream's place added.
 *
 * Stream i lands in d_dst (any byte address; at most cap bytes are used), one stream behind the other, each on a 32-byte boundary of the
 * buffer: [out_offset, out_offset + out_bytes) of its record; bytes outside every such range are not written.  A container whose status
 * is not M2V_DEMUX_OK has out_bytes 0, takes no room and no stamps, and its counters are 0; M2V_DEMUX_OVERFLOW: the stream did not fit
 * into cap behind those before it (m2v_demux_bound - the sum of the sizes, each rounded up to 32 - is always enough).  d_stamps (on an
 * 8-byte boundary; NULL with stamp_cap 0) receives one m2v_demux_stamp per PES packet, the containers' stamps one behind the other in
 * container order: stream i's begin at the sum of the pes_packets before it; those at or past stamp_cap are left out.
 *
 * The call blocks until the records are complete (one wait, as m2v_mux_device); m2v_demux_report pops them, oldest first (out NULL:
 * how many wait); they are dropped at the next m2v_demux_device.  M2V_E_STATE while a sequence is in progress or a resident call is in
 * flight; M2V_E_PARAM for an unknown kind, a `stream` out of range, no or more than 65535 containers.  Work buffers (16 bytes per
 * transport packet; 16 bytes per 9 bytes of a program stream) are allocated by the first call, by size, and freed with the handle.
 * m2v_demux_scan_tile: the bytes of a transport stream after which the kernels hand over to another workgroup.
 * Option "demux_blocks" (m2v_set_option): the most workgroups one launch of the demultiplexer's kernels has, 1 .. 4096; 0 (the default):
 * 4096.  They are shared out among a call's containers, and what a launch does not cover at once goes round the kernels' loops: the
 * result does not depend on it.  A caller that demultiplexes beside other work on the device can keep the footprint small with it; the
 * tests use it to send small containers round every loop.
 */
enum { M2V_DEMUX_OK = 0, M2V_DEMUX_SYNTAX = -2, M2V_DEMUX_OVERFLOW = -3, M2V_DEMUX_NOSTREAM = -4 };
typedef struct { uint64_t src_offset, src_bytes, out_offset, out_bytes, err_offset;
                 uint32_t pes_packets, packets, discontinuities, skipped, stream; int32_t status; } m2v_demux_stat;      /* 64 bytes */
typedef struct { uint64_t es_offset, pts, dts, src_offset; } m2v_demux_stamp;      /* 32 bytes; pts / dts = ~0 when absent; es_offset within the stream */
size_t m2v_demux_bound(const uint64_t *src_bytes, size_t nstreams);
int m2v_demux_device(m2v_enc *e, int kind, const void *d_src, const uint64_t *src_off, const uint64_t *src_bytes, size_t nstreams, int stream,
                     void *d_dst, size_t cap, void *d_stamps, size_t stamp_cap, void *hip_stream);
int m2v_demux_report(m2v_enc *e, m2v_demux_stat *out, size_t max);
int m2v_demux_scan_tile(void);

/*
 * Deinterlace on the device: woven 4:2:0 frames to progressive frames, the stage between m2v_decode_device and an encode (the encoder is
 * progressive only, and a source size - m2v_set_source_size - filters vertically across both fields).  d_src holds nframes frames of
 * width x height back to back, exactly as m2v_decode_device writes them (layout = M2V_420_I420 / YV12 / NV12 / NV21; frame_bytes =
 * w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2), rows without padding); the output frames have the same size and layout, nframes of them
 * (rate M2V_DEINT_FRAME_RATE) or 2 * nframes (M2V_DEINT_FIELD_RATE), back to back at d_dst.  Both pointers may be any byte address.
 * The call enqueues ONE launch for all frames, planes and outputs on hip_stream (NULL: the handle's stream) and returns without a host
 * wait; nothing has to be read back.  All offsets are computed in 64 bits.  What reads the output is ordered behind the launch by the
 * stream: an m2v_encode_resident420 on the same stream needs nothing else, a copy on another stream needs a wait of the caller's.  The
 * handle keeps no state of the call and allocates nothing for it.
 *
 * Planes.  Every plane is processed alone and bytewise: Y is h rows of w bytes, each I420 / YV12 chroma plane (h + 1) / 2 rows of
 * (w + 1) / 2 bytes, the NV12 / NV21 chroma plane (h + 1) / 2 rows of 2 * ((w + 1) / 2) bytes.  Row r of ANY plane belongs to the field
 * of parity r & 1, 0 being the top field: interlaced 4:2:0 as 13818-2 lays it out.  A plane with a single row is copied to every output.
 *
 * Fields.  The fields of a call form one sequence in time: F[k], k = 0 .. 2 * nframes - 1, lies in frame k >> 1 and has parity
 * order ^ (k & 1) (order: the parity of the field that is first in time, M2V_DEINT_TFF or M2V_DEINT_BFF, the same for the whole call).
 * A field index outside the call means the nearest field of the same parity inside it: k - 2 becomes k at the front, k + 1 becomes
 * k - 1 at the back, and so on.  Frame rate writes one frame for every even k, field rate one for every k, in order.
 *
 * The output for field k of parity p, in a plane of H >= 2 rows: a row y with (y & 1) == p is row y of frame k >> 1.  Any other row is
 * interpolated.  yc = y - 1 if that is >= 0, else y + 1; ye = y + 1 if that is < H, else y - 1 (a row missing at the plane's edge is
 * replaced by the one kept row beside it); c and e are the samples of frame k >> 1 in rows yc and ye, sp = (c + e + 1) >> 1.
 *   M2V_DEINT_LINE      the sample is sp.
 *   M2V_DEINT_ADAPTIVE  the sample is min(max(sp, d - m), d + m), with b and a the samples of row y in the frames that hold F[k - 1]
 *                       and F[k + 1], d = (b + a) >> 1, t0 = |b - a| >> 1, t1 = (|c' - c| + |e' - e|) >> 1 with c' and e' rows yc and
 *                       ye of the frame that holds F[k - 2], t2 the same against F[k + 2], m = max(t0, t1, t2).  The temporal core
 *                       of the familiar motion-adaptive filters: where nothing moves the other field is woven in, where something
 *                       moves the sample falls back to sp, and the width of the clamp is the motion found.  No threshold, no
 *                       edge-directed search.
 *   M2V_DEINT_BLEND     frame rate only, knows no parity: o[y] = (s[max(y - 1, 0)] + 2 * s[y] + s[min(y + 1, H - 1)] + 2) >> 2, frame
 *                       by frame.
 * A column of one plane, rows 0 2 4 6 8 10 12 14: LINE gives 0 2 4 6 8 10 12 12 (TFF) and 2 2 4 6 8 10 12 14 (BFF), BLEND
 * 1 2 4 6 8 10 12 14.
 *
 * M2V_E_PARAM for an unknown layout, mode, rate or order, for BLEND with FIELD_RATE, for width < 1, height < 2 or either above 16384,
 * and where the source range and the destination range overlap.  M2V_E_OVERFLOW where cap is below m2v_deinterlace_bound: not one byte
 * is written.  M2V_E_STATE while a sequence is in progress or a resident call is in flight, as m2v_decode_device.  nframes == 0 is
 * M2V_OK and launches nothing.  m2v_deinterlace_bound: the bytes a call writes, 0 for illegal arguments.  m2v_deinterlace_tile: the
 * bytes of a row and the rows after which the kernel hands over to another group of lanes (a test aims sizes at them).
 *
 * Out of scope: a per-picture record of top_field_first / progressive_frame / repeat_first_field from the decoder (the caller states the
 * order for the whole call), pulldown, edge-directed interpolation, 4:4:4 and RGB frames, deinterlacing as an automatic stage inside
 * the resident entries, and the batch entries.
 */
enum { M2V_DEINT_LINE = 0, M2V_DEINT_ADAPTIVE = 1, M2V_DEINT_BLEND = 2 };   /* mode  */
enum { M2V_DEINT_FRAME_RATE = 0, M2V_DEINT_FIELD_RATE = 1 };                 /* rate  */
enum { M2V_DEINT_TFF = 0, M2V_DEINT_BFF = 1 };                               /* order: parity of the field that is first in time */
int m2v_deinterlace_device(m2v_enc *e, const void *d_src, size_t nframes, int width, int height, int layout,
                           int mode, int rate, int order, void *d_dst, size_t cap, void *hip_stream);
unsigned long long m2v_deinterlace_bound(int width, int height, size_t nframes, int rate);   /* bytes written; 0 for illegal arguments */
int m2v_deinterlace_tile(int *cols, int *rows);   /* the kernel's tile, for tests, like m2v_decode_scan_tile */

/* Per-kernel statistics of the last m2v_encode_resident call with "profile" = 1.
 * kernel: 0 = macroblock kernel on P frames, 1 = macroblock kernel on I frames,
 * 2 = strip mode's final assembly (k_strip_layout + k_strip_assemble), 3 = slice assembly (k_assemble), 4 = scans,
 * 5 = the cut detector of option "scene_cut" (k_mbsum + k_scene_judge), 6 = the reconstruction out of m2v_set_recon_out (k_recon_out).
 * Returns launches; *ms = summed duration, *units = luma pixels processed. */
int m2v_kernel_stats(const m2v_enc *e, int kernel, double *ms, double *units);

/*
 * Stage-level introspection for the parity tests (not part of the port contract): copies an
 * intermediate of the last m2v_encode_resident call to host memory.  what = 1 and a complete what = 3 need the
 * debug build of the library (libm2v_mi355x_dbg.so, compiled with -DM2V_DEBUG, option "keep_recon"); the shipped
 * library carries no dump code in its kernels and answers M2V_E_STATE for what = 1.
 *   what: 0 = mb info  uint32 [frames][mbs]  (bit0 inter, bits1-6 cbp, bits8-15 mvx, bits16-23 mvy, two's complement)
 *         1 = levels   int16  [frames][mbs][6][64] (zig-zag order)
 *         2 = mb bits  uint32 [frames][mbs]
 *         3 = recon    uint8  [frames][W*H*3/2]  (only frames that are referenced later; others 0)
 *         4 = the expanded 4:4:4 input of the last m2v_encode_resident420 / m2v_encode_resident_rgb call's last chunk (the converted
 *             planes after an RGB call), uint8 [frames][3*W*H]: a plain copy of
 *             the handle's own buffer (either library answers it; M2V_E_STATE before the first such call has completed).  With a frame
 *             size set (m2v_set_frame_size) the planes are the padded ones, and m2v_encode_resident's frames pass through that buffer too
 *         5 = mb aux   uint32 [frames][mbs][4]: the record k_mb leaves next to the info word (either library).  Word 0 = bits of the
 *             slot's first segment | second << 16, word 1 = bits of the third | DC level of V << 16, word 2 = DC levels of the first |
 *             last luma tile << 16, word 3 = DC level of U.  The three segment lengths add up to the bits kept in the macroblock's slot.
 * Returns bytes copied or a negative error.
 */
long long m2v_debug_read(m2v_enc *e, int what, void *dst, size_t cap);

/* Text of the last failure on this handle; with e == NULL, why the last m2v_create on the calling thread failed. */
const char *m2v_last_error(const m2v_enc *e);

/*
 * The product's constant tables, readable without a GPU (tests/test_abi.py compares them with the oracle's and
 * with the RTL's assign lines): which 0 = DCT basis [i][j] (RTL:2020-2027), 1 = intra quantiser matrix (RTL:2080-2087),
 * 2 = zig-zag position (RTL:2439-2446), 3 = motion code i (len << 8 | code, RTL:2500-2519), 4 = coded block pattern i,
 * 5 = DC size code (len << 16 | code) of component i, size j, 6 = run/level code of run i, level j (0 = escape);
 * 16 + p (p = 0 .. 8) = the macroblock position that block i of a launch of j blocks works on with option "cu_pack" = p
 * (a permutation of 0 .. j-1 for every j and p).
 */
int m2v_debug_table(int which, int i, int j);

#ifdef __cplusplus
}
#endif
#endif
