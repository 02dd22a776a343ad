// m2v_tb — file-to-file driver over the C-ABI; the counterpart of SIM/tb_mpeg2encoder.v.
//
//   m2v_tb [-XL n] [-YL n] [-VL n] [-Q n] [-p pframes] [-d device] [-bubbles] [-conformant] [-ps] [-ts] [-devmux]
//          [-i420 | -yv12 | -nv12 | -nv21 | -rgb24 | -bgr24 | -rgbx | -bgrx | -xrgb | -xbgr | -rgbp] [-matrix bt601|bt709|bt601f|bt709f]
//          [-pad | -truesize] [-stats] [-qgop q0,q1,...] [-istart n0,n1,...] [-scenecut T] [-recon out.yuv [-reconfmt i420|yv12|nv12|nv21]]
//          [-fps N/D] [-aspect 1:1|4:3|16:9|2.21:1] [-bitrate B] [-vbv K] [-colour bt601|bt709|P,T,M] [-repeat-headers]
//          [-scale SWxSH [-filter triangle|area]]
//          in.yuv W H out.m2v  [in2.yuv W2 H2 out2.m2v ...]
//   m2v_tb -decode in.m2v out.yuv [-reconfmt i420|yv12|nv12|nv21] [-mode iso|module] [-syntax module|main [-bpictures] [-interlaced] [-extended [-mbtools [-fieldpictures [-join head|tail|both] [-conceal]]]]] [-container ts|ps [-pid N]] [-deint line|adaptive|blend [-fieldrate] [-bff]] [-d device]
//   m2v_tb -demux ts|ps in.ts out.m2v [-pid N] [-d device]
//
// -demux: the video elementary stream of a transport or program stream, demultiplexed on the device (m2v_demux_device), into out.m2v, with
// one line about the container; -pid N: the PID / stream_id to take (default: found in the container).  -decode ... -container ts|ps:
// in.m2v is such a container; it is demultiplexed on the device and the stream decoded from where it lands, without a trip to the host.
// A container the demultiplexer refuses ends with its status and the offset of the packet or unit in error, exit status 1.
// -decode: the other way - the elementary stream of in.m2v decoded on the device (m2v_decode_device: a probe for the size, then the
// decode) into 4:2:0 frames of the header's size in -reconfmt (default i420), frame behind frame in out.yuv.  -mode iso (default): the
// standard's reconstruction, for streams coded with -conformant; -mode module: the module's own loop, for every other stream of this
// encoder.  -syntax main: option "decode_syntax" = M2V_SYNTAX_MAIN, Main-Profile I / P streams of any encoder (-mode iso only);
// -bpictures with it: option "decode_b_pictures" = 1, B pictures too, the frames written in display order.
// -extended with it: option "decode_extended" = 1, several slices a row, slice header extras, quant_matrix_extension, composite_display_flag 1.
// -mbtools with -extended: option "decode_mb_tools" = 1, Table B-15, concealment motion vectors and dual prime.
// -fieldpictures with -interlaced -extended -mbtools: option "decode_field_pictures" = 1, picture_structure 1 / 2 too, two field pictures a frame.
// -join head|tail|both with -fieldpictures: option "decode_join" = 1 / 2 / 3, a stream cut from a broadcast; prints the join record.
// -conceal with -fieldpictures: option "decode_conceal" = 1, damaged slices dropped and their rows patched; prints the report.
// -interlaced with it: option "decode_interlaced" = 1, frame pictures with field prediction and field DCT too, one frame per picture.
// -deint line|adaptive|blend: the decoded frames are deinterlaced on the device (m2v_deinterlace_device) before they are written, a frame
// per frame or with -fieldrate a frame per field (not with blend), top field first or with -bff bottom field first.
// A stream the decoder refuses ends with its status and the offset of the unit in error, exit status 1.
// -pad: W, H are any size from 49 up; the files hold frames of that size in the chosen format, which are padded to whole macroblocks on
// the device (m2v_set_frame_size) - the stream is the module's for the padded frames.  -truesize: -pad, and the stream's headers say
// W x H instead of the padded size (M2V_HEADER_TRUE; not the module's header).  Neither goes with -bubbles: there are no partial macroblocks.
// -i420 / -yv12 / -nv12 / -nv21: the input files hold 4:2:0 frames of W*H*3/2 bytes in that layout (what ordinary tools write) instead
// of the testbench's planar 4:4:4 frames; they go in through m2v_push_frames420.  At most one of the four.
// -rgb24 / -bgr24 / -rgbx / -bgrx / -xrgb / -xbgr / -rgbp: the input files (.rgb, .bgra, ...) hold RGB frames of W*H*3 or W*H*4 bytes in that
// layout (M2V_RGB_*); they go in through m2v_push_rgb and are converted on the device with -matrix (default bt601).  At most one of
// the eleven layout options.
// -stats: the encoder's option "stats"; after each video one line per picture - frame, type, PSNR of Y, U, V against the source, intra /
// inter macroblocks, bits of the macroblock layer, bytes of the picture in the stream (m2vc_scan) - and a mean / min summary line.
// The PSNR is the module's reconstruction against the 4:2:0 source it codes, over the source's size under -pad (m2v_picture_stats in
// include/m2v_mi355x.h says what that means without -conformant).
// -qgop 1,4,3: a level per GOP (m2v_set_gop_levels): GOP k of every video at the k-th value, the last value for the GOPs beyond; NOT
// the module's behaviour, -Q stays the handle's level.
// -istart 5,9,40: a GOP also starts at each of these frame numbers of every video (m2v_set_gop_starts; strictly ascending); NOT the
// module's behaviour.  The port path takes it.
// -scenecut T: option "scene_cut" = T, 1..65280: a GOP also starts where the device finds a scene cut; NOT the module's behaviour.  The
// detector belongs to the resident entries, so with this flag - and only with it - every file's frames are staged in device memory
// whole and encoded by one m2v_encode_resident* call instead of going through the port.  Does not go with -bubbles.
// -recon out.yuv: the reconstructed pictures of every video, frame behind frame, as 4:2:0 frames of W x H (the file's size under -pad too)
// in -reconfmt (default i420): m2v_set_recon_out, read back after each video - a file for ffplay -f rawvideo or tools/m2v_stats.py --yuv.
// The buffer is the resident entries', so it needs the resident mode that -scenecut selects (-scenecut 65280 never finds a cut).
// -scale SWxSH: the files hold frames of SW x SH in the chosen format; W H on the command line are the picture size they are resampled
// to on the device (m2v_set_source_size) with -filter (default triangle), under -pad any size from 49 up.  The resident entries resample,
// so the flag selects the resident mode that -scenecut selects.  Does not go with -bubbles.
// -fps N/D, -aspect A, -bitrate B, -vbv K, -colour C, -repeat-headers: what the stream says about itself (m2v_set_stream_desc); NOT the
// module's behaviour.  N/D: a rational equal to a frame rate of ISO/IEC 13818-2 table 6-4 (24000/1001, 24, 25, 30000/1001, 30, 50,
// 60000/1001, 60; "/D" may be left out), which the GOP headers' time codes then count at; B: bit/s, rounded up to units of 400; K: the
// vbv buffer size in its own units of 16384 bits; C: bt601 (5,5,5), bt709 (1,1,1) or colour_primaries,transfer_characteristics,
// matrix_coefficients, each 1..255 - the label only, -matrix is what converts; -repeat-headers: the sequence headers again in front of every
// GOP after the first, so that a player can start there.  A bad value ends with the usage text and exit status 2 before the device is touched.
// -conformant switches the encoder's option "conformant" on (ISO reconstruction loop; NOT byte-identical to the RTL).
// -ps / -ts additionally write out.m2v.mpg / out.m2v.ts: the same elementary stream in an MPEG-2 program / transport
// stream (include/m2v_container.h), so the result plays in an ordinary player.  -devmux: those files come from the device muxer
// (m2v_mux_device over the stream in device memory) instead of the CPU's - the same bytes.
//
// Like the testbench it encodes the listed videos back to back on ONE encoder instance (TB:150:
// "verify the module can end a sequence and start the next"), pushes only the complete frames of
// each file (TB:220), 4 pixels per beat in raster order (TB:224-229), pulses stop with i_en = 0
// (TB:249-252) and writes o_data byte 0 first (TB:260-262).  Defaults are the testbench's:
// XL=7 YL=6 VECTOR_LEVEL=3 Q_LEVEL=2 i_pframes_count=23 (TB:23-24, 98-106).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/m2v_container.h"
#include "../../include/m2v_mi355x.h"

static bool read_file(const char *path, std::vector<uint8_t> &bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + n);
    fclose(f);
    return true;
}

// the container of n bytes at d_src through m2v_demux_device into a new allocation *d_es, zeroed first so that the stream can be handed
// on with the zero padding to a whole 32-byte word that a muxer drops behind sequence_end_code: 0, or 1 with the reason on stderr
static int demux_to_device(m2v_enc *e, int kind, int pid, const void *d_src, size_t n, const char *name, void **d_es, m2v_demux_stat *r)
{
    const uint64_t off = 0, bytes = n;
    const size_t cap = m2v_demux_bound(&bytes, 1);
    if (hipMalloc(d_es, cap + 32) != hipSuccess || hipMemset(*d_es, 0, cap + 32) != hipSuccess) { fprintf(stderr, "m2v_tb: no device memory for the stream\n"); return 1; }
    if (m2v_demux_device(e, kind, d_src, &off, &bytes, 1, pid, *d_es, cap, nullptr, 0, nullptr) != M2V_OK || m2v_demux_report(e, r, 1) != 1) {
        fprintf(stderr, "m2v_demux_device: %s\n", m2v_last_error(e));
        return 1;
    }
    if (r->status != M2V_DEMUX_OK) {
        fprintf(stderr, "%s: not demultiplexed: status %d%s, the packet or unit at byte %llu\n", name, (int)r->status,
                r->status == M2V_DEMUX_NOSTREAM ? " (no video stream)" : "", (unsigned long long)r->err_offset);
        return 1;
    }
    return 0;
}

static int container_kind(const char *v) { return !strcmp(v, "ts") ? M2V_MUX_TS : !strcmp(v, "ps") ? M2V_MUX_PS : 0; }

static int demux_main(int argc, char **argv)
{
    const int kind = container_kind(argv[2]);
    const char *in = argv[3], *out = argv[4];
    int pid = -1, dev = 0;
    bool bad = !kind;
    for (int i = 5; i < argc; i += 2) {
        if (i + 1 < argc && !strcmp(argv[i], "-pid")) pid = (int)strtol(argv[i + 1], nullptr, 0);
        else if (i + 1 < argc && !strcmp(argv[i], "-d")) dev = atoi(argv[i + 1]);
        else bad = true;
    }
    if (bad) { fprintf(stderr, "m2v_tb -demux ts|ps in out.m2v [-pid N] [-d device]\n"); return 2; }
    std::vector<uint8_t> box;
    if (!read_file(in, box)) return 1;
    int err = 0;
    m2v_enc *e = m2v_create(7, 7, 3, 2, dev, &err);
    if (!e) { fprintf(stderr, "m2v_create: %s\n", m2v_last_error(nullptr)); return 1; }
    void *d_src = nullptr, *d_es = nullptr;
    m2v_demux_stat r;
    int rc = 1;
    if (hipMalloc(&d_src, box.size() + 1) != hipSuccess || hipMemcpy(d_src, box.data(), box.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fprintf(stderr, "m2v_tb: no device memory for the container\n");
    } else if (demux_to_device(e, kind, pid, d_src, box.size(), in, &d_es, &r) == 0) {
        std::vector<uint8_t> es((size_t)r.out_bytes);
        FILE *o = fopen(out, "wb");
        if (hipMemcpy(es.data(), (const uint8_t *)d_es + r.out_offset, es.size(), hipMemcpyDeviceToHost) != hipSuccess || !o || fwrite(es.data(), 1, es.size(), o) != es.size()) {
            fprintf(stderr, "m2v_tb: cannot write %s\n", out);
        } else {
            printf("%s: stream 0x%x, %u PES packets in %u %s, %u skipped, %u discontinuities -> %s (%llu bytes)\n", in, r.stream, r.pes_packets, r.packets,
                   kind == M2V_MUX_TS ? "packets" : "packs", r.skipped, r.discontinuities, out, (unsigned long long)r.out_bytes);
            rc = 0;
        }
        if (o) fclose(o);
    }
    if (d_src) (void)hipFree(d_src);
    if (d_es) (void)hipFree(d_es);
    m2v_destroy(e);
    return rc;
}

static int decode_main(int argc, char **argv)
{
    const char *in = argv[2], *out = argv[3];
    int layout = M2V_420_I420, mode = M2V_DEC_ISO, dev = 0, container = 0, pid = -1, syntax = M2V_SYNTAX_MODULE, bpictures = 0, interlaced = 0, extended = 0, mbtools = 0, fieldpictures = 0, join = 0, conceal = 0, deint = -1, fieldrate = 0, bff = 0;
    bool bad = false;
    for (int i = 4; i < argc; ++i) {
        const char *v = i + 1 < argc ? argv[i + 1] : "";
        if (!strcmp(argv[i], "-reconfmt")) {
            const char *names[4] = {"i420", "yv12", "nv12", "nv21"};
            for (layout = 0; layout < 4 && strcmp(v, names[layout]); ++layout) {}
            ++i;
        } else if (!strcmp(argv[i], "-mode")) {
            mode = !strcmp(v, "iso") ? M2V_DEC_ISO : !strcmp(v, "module") ? M2V_DEC_MODULE : -1;
            ++i;
        } else if (!strcmp(argv[i], "-syntax")) {
            syntax = !strcmp(v, "main") ? M2V_SYNTAX_MAIN : !strcmp(v, "module") ? M2V_SYNTAX_MODULE : -1;
            bad = bad || syntax < 0;
            ++i;
        } else if (!strcmp(argv[i], "-bpictures")) {
            bpictures = 1;
        } else if (!strcmp(argv[i], "-interlaced")) {
            interlaced = 1;
        } else if (!strcmp(argv[i], "-extended")) {
            extended = 1;
        } else if (!strcmp(argv[i], "-mbtools")) {
            mbtools = 1;
        } else if (!strcmp(argv[i], "-fieldpictures")) {
            fieldpictures = 1;
        } else if (!strcmp(argv[i], "-conceal")) {
            conceal = 1;
        } else if (!strcmp(argv[i], "-join")) {
            join = !strcmp(v, "head") ? M2V_JOIN_HEAD : !strcmp(v, "tail") ? M2V_JOIN_TAIL : !strcmp(v, "both") ? (M2V_JOIN_HEAD | M2V_JOIN_TAIL) : -1;
            bad = bad || join < 0;
            ++i;
        } else if (!strcmp(argv[i], "-deint")) {
            deint = !strcmp(v, "line") ? M2V_DEINT_LINE : !strcmp(v, "adaptive") ? M2V_DEINT_ADAPTIVE : !strcmp(v, "blend") ? M2V_DEINT_BLEND : -1;
            bad = bad || deint < 0;
            ++i;
        } else if (!strcmp(argv[i], "-fieldrate")) {
            fieldrate = 1;
        } else if (!strcmp(argv[i], "-bff")) {
            bff = 1;
        } else if (!strcmp(argv[i], "-d")) {
            dev = atoi(v);
            ++i;
        } else if (!strcmp(argv[i], "-container")) {
            container = container_kind(v);
            bad = bad || !container;
            ++i;
        } else if (!strcmp(argv[i], "-pid")) {
            pid = (int)strtol(v, nullptr, 0);
            ++i;
        } else {
            bad = true;
        }
    }
    if (bad || (pid >= 0 && !container) || ((fieldrate || bff) && deint < 0) || (fieldrate && deint == M2V_DEINT_BLEND)) {
        fprintf(stderr, "m2v_tb -decode in.m2v out.yuv [-reconfmt i420|yv12|nv12|nv21] [-mode iso|module] [-syntax module|main [-bpictures] [-interlaced] [-extended [-mbtools [-fieldpictures [-join head|tail|both] [-conceal]]]]] [-container ts|ps [-pid N]] [-deint line|adaptive|blend [-fieldrate] [-bff]] [-d device]\n");
        return 2;
    }
    std::vector<uint8_t> es;
    if (!read_file(in, es)) return 1;
    int err = 0;
    m2v_enc *e = m2v_create(7, 7, 3, 2, dev, &err);
    if (!e) { fprintf(stderr, "m2v_create: %s\n", m2v_last_error(nullptr)); return 1; }
    void *d_in = nullptr, *d_box = nullptr, *d_out = nullptr, *d_prog = nullptr;
    const void *d_es = nullptr;
    size_t es_bytes = es.size();
    m2v_decode_stat r;
    m2v_demux_stat dr;
    int rc = 1;
    if (hipMalloc(&d_in, es.size() + 1) != hipSuccess || hipMemcpy(d_in, es.data(), es.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fprintf(stderr, "m2v_tb: no device memory for the stream\n");
    } else if (!container) {
        d_es = d_in;
    } else if (demux_to_device(e, container, pid, d_in, es.size(), in, &d_box, &dr) == 0) {
        d_es = (const uint8_t *)d_box + dr.out_offset;      // the stream stays where the demultiplexer left it
        es_bytes = ((size_t)dr.out_bytes + 31) / 32 * 32;   // (the decoder's definition wants whole words: the zeros are there)
    }
    if (!d_es) {
        // (said)
    } else if (m2v_set_option(e, "decode_syntax", syntax) != M2V_OK || m2v_set_option(e, "decode_b_pictures", bpictures) != M2V_OK ||
               m2v_set_option(e, "decode_interlaced", interlaced) != M2V_OK || m2v_set_option(e, "decode_extended", extended) != M2V_OK ||
               m2v_set_option(e, "decode_mb_tools", mbtools) != M2V_OK || m2v_set_option(e, "decode_field_pictures", fieldpictures) != M2V_OK ||
               m2v_set_option(e, "decode_join", join) != M2V_OK || m2v_set_option(e, "decode_conceal", conceal) != M2V_OK) {
        fprintf(stderr, "m2v_set_option: %s\n", m2v_last_error(e));
    } else if (m2v_decode_device(e, d_es, es_bytes, nullptr, 0, layout, mode, nullptr) != M2V_OK || m2v_decode_report(e, &r) != M2V_OK) {
        fprintf(stderr, "m2v_decode_device: %s\n", m2v_last_error(e));
    } else if (r.status == M2V_DEC_OK && hipMalloc(&d_out, (size_t)r.out_bytes + 1) != hipSuccess) {
        fprintf(stderr, "m2v_tb: no device memory for %llu bytes of frames\n", (unsigned long long)r.out_bytes);
    } else if (r.status == M2V_DEC_OK && (m2v_decode_device(e, d_es, es_bytes, d_out, (size_t)r.out_bytes, layout, mode, nullptr) != M2V_OK ||
                                          m2v_decode_report(e, &r) != M2V_OK)) {
        fprintf(stderr, "m2v_decode_device: %s\n", m2v_last_error(e));
    } else if (r.status != M2V_DEC_OK) {
        fprintf(stderr, "%s: not decoded: status %d, the unit at byte %llu\n", in, (int)r.status, (unsigned long long)r.err_offset);
    } else if (deint >= 0 && r.pictures && hipMalloc(&d_prog, (size_t)r.out_bytes * (fieldrate ? 2 : 1)) != hipSuccess) {
        fprintf(stderr, "m2v_tb: no device memory for %llu bytes of deinterlaced frames\n", (unsigned long long)r.out_bytes * (fieldrate ? 2 : 1));
    } else if (deint >= 0 && r.pictures && m2v_deinterlace_device(e, d_out, r.pictures, (int)r.width, (int)r.height, layout, deint, fieldrate, bff, d_prog,
                                                                  (size_t)r.out_bytes * (fieldrate ? 2 : 1), nullptr) != M2V_OK) {
        fprintf(stderr, "m2v_deinterlace_device: %s\n", m2v_last_error(e));
    } else if (deint >= 0 && hipDeviceSynchronize() != hipSuccess) {      // (the entry does not wait, and the handle's stream does not block the copy below)
        fprintf(stderr, "m2v_tb: the deinterlacer's launch failed\n");
    } else {
        const bool prog = deint >= 0 && r.pictures;
        std::vector<uint8_t> frames((size_t)r.out_bytes * (prog && fieldrate ? 2 : 1));
        FILE *o = fopen(out, "wb");
        if (hipMemcpy(frames.data(), prog ? d_prog : d_out, frames.size(), hipMemcpyDeviceToHost) != hipSuccess || !o || fwrite(frames.data(), 1, frames.size(), o) != frames.size()) {
            fprintf(stderr, "m2v_tb: cannot write %s\n", out);
        } else {
            printf("%s: %u pictures of %u x %u, %u GOPs -> %s (%llu bytes)\n", in, r.pictures, r.width, r.height, r.gops, out, (unsigned long long)frames.size());
            if (prog) printf("%s: deinterlaced on the device, mode %d, %s, %s field first\n", in, deint, fieldrate ? "a frame per field" : "a frame per frame", bff ? "bottom" : "top");
            m2v_decode_join j;
            if (join && m2v_decode_join_report(e, &j) == M2V_OK)
                printf("%s: joined at byte %llu, read up to byte %llu of %llu; %u frames dropped in front, %u behind\n", in, (unsigned long long)j.join_offset,
                       (unsigned long long)j.tail_offset, (unsigned long long)r.es_bytes, j.dropped_leading, j.dropped_trailing);
            m2v_decode_conceal c;
            if (conceal && m2v_decode_conceal_report(e, &c) == M2V_OK)
                printf("%s: %u slices dropped, %u rows concealed (%u grey) in %u pictures, the first at byte %llu\n", in, c.bad_slices, c.concealed_rows, c.grey_rows,
                       c.damaged_pictures, (unsigned long long)c.first_offset);
            rc = 0;
        }
        if (o) fclose(o);
    }
    if (d_in) (void)hipFree(d_in);
    if (d_box) (void)hipFree(d_box);
    if (d_out) (void)hipFree(d_out);
    if (d_prog) (void)hipFree(d_prog);
    m2v_destroy(e);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "-decode")) return decode_main(argc, argv);
    if (argc >= 5 && !strcmp(argv[1], "-demux")) return demux_main(argc, argv);
    int XL = 7, YL = 6, VL = 3, Q = 2, pf = 23, dev = 0, bubbles = 0, conformant = 0, want_ps = 0, want_ts = 0, layout420 = -1, layouts = 0, rgb = -1, matrix = M2V_RGB_BT601,
        bad_matrix = 0, pad = 0, truesize = 0, stats = 0, reconfmt = M2V_420_I420, devmux = 0;
    const char *recon = nullptr;
    long long scenecut = 0;
    int ssw = 0, ssh = 0, filter = M2V_SCALE_TRIANGLE, bad_scale = 0;
    std::vector<uint8_t> qgop;
    std::vector<uint32_t> istart;
    bool have_istart = false;
    m2v_stream_desc desc;
    m2v_stream_desc_module(&desc);
    int bad_desc = 0;
    int i = 1;
    for (; i < argc && argv[i][0] == '-'; ++i) {
        if (!strcmp(argv[i], "-bubbles")) { bubbles = 1; continue; }
        if (!strcmp(argv[i], "-conformant")) { conformant = 1; continue; }
        if (!strcmp(argv[i], "-ps")) { want_ps = 1; continue; }
        if (!strcmp(argv[i], "-ts")) { want_ts = 1; continue; }
        if (!strcmp(argv[i], "-devmux")) { devmux = 1; continue; }
        if (!strcmp(argv[i], "-pad")) { pad = 1; continue; }
        if (!strcmp(argv[i], "-stats")) { stats = 1; continue; }
        if (!strcmp(argv[i], "-truesize")) { pad = truesize = 1; continue; }
        if (!strcmp(argv[i], "-repeat-headers")) { desc.repeat_headers = 1; continue; }
        if (!strcmp(argv[i], "-i420")) { layout420 = M2V_420_I420; ++layouts; continue; }
        if (!strcmp(argv[i], "-yv12")) { layout420 = M2V_420_YV12; ++layouts; continue; }
        if (!strcmp(argv[i], "-nv12")) { layout420 = M2V_420_NV12; ++layouts; continue; }
        if (!strcmp(argv[i], "-nv21")) { layout420 = M2V_420_NV21; ++layouts; continue; }
        static const char *const rgb_opts[] = {"-rgb24", "-bgr24", "-rgbx", "-bgrx", "-xrgb", "-xbgr", "-rgbp"};
        int k = 0;
        for (; k < 7 && strcmp(argv[i], rgb_opts[k]); ++k) {}
        if (k < 7) { rgb = k; ++layouts; continue; }
        if (i + 1 >= argc) break;                                   // (an option that takes a value is never the last argument)
        if (!strcmp(argv[i], "-qgop")) {
            for (const char *c = argv[i + 1]; *c; ++c)
                if (*c >= '0' && *c <= '9') qgop.push_back((uint8_t)(*c - '0'));
                else if (*c != ',') qgop.push_back(0);              // (not a level: m2v_set_gop_levels says so)
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-istart")) {
            have_istart = true;
            for (const char *c = argv[i + 1]; *c;) {
                if (*c >= '0' && *c <= '9') { char *end = nullptr; istart.push_back((uint32_t)strtoul(c, &end, 10)); c = end; }
                else if (*c == ',') ++c;
                else { istart.assign(2, 0); break; }                // (not a list: m2v_set_gop_starts says so)
            }
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-fps")) {
            char *end = nullptr;
            const unsigned long long num = strtoull(argv[i + 1], &end, 10);
            unsigned long long den = 1;
            bool ok = end != argv[i + 1] && argv[i + 1][0] != '-';
            if (ok && *end == '/') { const char *d = end + 1; den = strtoull(d, &end, 10); ok = end != d && *d != '-'; }
            const int code = ok && !*end && num <= 0xFFFFFFFFull && den <= 0xFFFFFFFFull ? m2v_frame_rate_code((uint32_t)num, (uint32_t)den) : -1;
            if (code < 0) bad_desc = 1; else desc.frame_rate_code = (uint32_t)code;
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-aspect")) {
            static const char *const names[] = {"1:1", "4:3", "16:9", "2.21:1"};
            for (k = 0; k < 4 && strcmp(argv[i + 1], names[k]); ++k) {}
            if (k < 4) desc.aspect_ratio_information = (uint32_t)k + 1; else bad_desc = 1;
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-bitrate") || !strcmp(argv[i], "-vbv")) {
            const bool rate = argv[i][1] == 'b';
            char *end = nullptr;
            const unsigned long long v = strtoull(argv[i + 1], &end, 10);
            const unsigned long long units = rate ? (v + 399) / 400 : v;
            if (end == argv[i + 1] || *end || argv[i + 1][0] == '-' || v > (1ull << 40) || units < (rate ? 1u : 0u) || units > (rate ? 0x3FFFFFFFull : 0x3FFFFull)) bad_desc = 1;
            else (rate ? desc.bit_rate_400 : desc.vbv_buffer_size_16k) = (uint32_t)units;
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-colour")) {
            unsigned c[3] = {0, 0, 0};
            char tail = 0;
            if (!strcmp(argv[i + 1], "bt601")) c[0] = c[1] = c[2] = 5;
            else if (!strcmp(argv[i + 1], "bt709")) c[0] = c[1] = c[2] = 1;
            else if (sscanf(argv[i + 1], "%3u,%3u,%3u%c", &c[0], &c[1], &c[2], &tail) != 3) c[0] = 0;
            if (c[0] < 1 || c[0] > 255 || c[1] < 1 || c[1] > 255 || c[2] < 1 || c[2] > 255) bad_desc = 1;
            else { desc.colour_primaries = c[0]; desc.transfer_characteristics = c[1]; desc.matrix_coefficients = c[2]; }
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-scenecut")) { scenecut = atoll(argv[i + 1]); ++i; continue; }
        if (!strcmp(argv[i], "-scale")) {
            char tail = 0;
            if (sscanf(argv[i + 1], "%6dx%6d%c", &ssw, &ssh, &tail) != 2 || ssw < 1 || ssh < 1 || ssw > 16384 || ssh > 16384) bad_scale = 1;
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-filter")) {
            if (!strcmp(argv[i + 1], "triangle")) filter = M2V_SCALE_TRIANGLE;
            else if (!strcmp(argv[i + 1], "area")) filter = M2V_SCALE_AREA;
            else bad_scale = 1;
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-recon")) { recon = argv[i + 1]; ++i; continue; }
        if (!strcmp(argv[i], "-reconfmt")) {
            static const char *const names[] = {"i420", "yv12", "nv12", "nv21"};
            for (k = 0; k < 4 && strcmp(argv[i + 1], names[k]); ++k) {}
            reconfmt = k;                                           // (4 = not a layout: m2v_set_recon_out says so)
            ++i;
            continue;
        }
        if (!strcmp(argv[i], "-matrix")) {
            static const char *const names[] = {"bt601", "bt709", "bt601f", "bt709f"};
            for (k = 0; k < 4 && strcmp(argv[i + 1], names[k]); ++k) {}
            if (k < 4) matrix = k; else bad_matrix = 1;
            ++i;
            continue;
        }
        int v = atoi(argv[i + 1]);
        if (!strcmp(argv[i], "-XL")) XL = v; else if (!strcmp(argv[i], "-YL")) YL = v;
        else if (!strcmp(argv[i], "-VL")) VL = v; else if (!strcmp(argv[i], "-Q")) Q = v;
        else if (!strcmp(argv[i], "-p")) pf = v; else if (!strcmp(argv[i], "-d")) dev = v;
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        ++i;
    }
    if ((argc - i) < 4 || (argc - i) % 4 || layouts > 1 || bad_matrix || bad_desc || bad_scale || ((layouts || pad || scenecut || ssw) && bubbles)) {          // (there are no 4:2:0 or RGB beats)
        fprintf(stderr, "usage: %s [-XL n] [-YL n] [-VL n] [-Q n] [-p pframes] [-d dev] [-i420 | -yv12 | -nv12 | -nv21 | -rgb24 | -bgr24 | -rgbx | -bgrx |"
                        " -xrgb | -xbgr | -rgbp] [-matrix bt601|bt709|bt601f|bt709f] [-pad | -truesize] [-stats] [-qgop q0,q1,...] [-istart n0,n1,...] [-scenecut T] [-recon out.yuv [-reconfmt i420|yv12|nv12|nv21]]"
                        " [-fps N/D] [-aspect 1:1|4:3|16:9|2.21:1] [-bitrate bit/s] [-vbv units of 16384 bits] [-colour bt601|bt709|P,T,M] [-repeat-headers] [-scale SWxSH [-filter triangle|area]] [-ps] [-ts] [-devmux]"
                        " in.yuv W H out.m2v ...\n"
                        "  -fps takes a frame rate of ISO/IEC 13818-2 table 6-4: 24000/1001, 24, 25, 30000/1001, 30, 50, 60000/1001, 60\n"
                        "  -scenecut T stages every file's frames in device memory and encodes them with one resident call (the detector needs it)\n"
                        "  -scale SWxSH: the files hold frames of SW x SH, resampled on the device to W x H; it selects the resident mode too\n", argv[0]);
        return 2;
    }
    const bool resident = scenecut || ssw;
    if (recon && !resident) {
        fprintf(stderr, "*** -recon needs the resident mode: the reconstruction is written to device memory by the resident entries, and only -scenecut T "
                        "stages the frames there (-scenecut 65280 never finds a cut)\n");
        return 2;
    }
    FILE *fr = nullptr;
    if (recon && !(fr = fopen(recon, "wb"))) { printf("*** couldn't open %s\n", recon); return 1; }
    int err = 0;
    m2v_enc *e = m2v_create(XL, YL, VL, Q, dev, &err);
    if (!e) { fprintf(stderr, "*** m2v_create failed (%d): an MI355X is required, there is no CPU fallback\n", err); return 1; }
    if (conformant) m2v_set_option(e, "conformant", 1);
    if (stats && m2v_set_option(e, "stats", 1) < 0) { fprintf(stderr, "*** m2v_set_option(stats): %s\n", m2v_last_error(e)); return 1; }
    if (!qgop.empty() && m2v_set_gop_levels(e, qgop.data(), qgop.size()) < 0) { fprintf(stderr, "*** m2v_set_gop_levels: %s\n", m2v_last_error(e)); return 1; }
    if (have_istart && m2v_set_gop_starts(e, istart.data(), istart.size()) < 0) { fprintf(stderr, "*** m2v_set_gop_starts: %s\n", m2v_last_error(e)); return 1; }
    if (m2v_set_stream_desc(e, &desc) < 0) { fprintf(stderr, "*** m2v_set_stream_desc: %s\n", m2v_last_error(e)); return 1; }
    if (scenecut && m2v_set_option(e, "scene_cut", scenecut) < 0) { fprintf(stderr, "*** m2v_set_option(scene_cut): %s\n", m2v_last_error(e)); return 1; }
    if (ssw && m2v_set_source_size(e, ssw, ssh, filter) < 0) { fprintf(stderr, "*** m2v_set_source_size: %s\n", m2v_last_error(e)); return 1; }
    int num_video = 0;
    for (; i + 3 < argc; i += 4) {
        ++num_video;
        const char *in = argv[i], *out = argv[i + 3];
        const int xsize = atoi(argv[i + 1]), ysize = atoi(argv[i + 2]);
        printf("start to encode video %d (%4dx%4d)\n", num_video, xsize, ysize);
        FILE *fi = fopen(in, "rb");
        if (!fi) { printf("*** couldn't open input file\n"); return 1; }                       // TB:175-180
        FILE *fo = fopen(out, "wb");
        if (!fo) { printf("*** couldn't open output file\n"); return 1; }                      // TB:182-187
        uint32_t xs16 = (uint32_t)xsize / 16, ys16 = (uint32_t)ysize / 16;
        if (pad) {
            if (xsize < 49 || xsize > (16 << XL)) { printf("*** xsize=%4d is invalid, which must in range [49,%4d] with -pad\n", xsize, 16 << XL); return 1; }
            if (ysize < 49 || ysize > (16 << YL)) { printf("*** ysize=%4d is invalid, which must in range [49,%4d] with -pad\n", ysize, 16 << YL); return 1; }
            if (m2v_fit_size(xsize, ysize, &xs16, &ys16) < 0 || m2v_set_frame_size(e, xsize, ysize, truesize ? M2V_HEADER_TRUE : M2V_HEADER_MODULE) < 0) {
                fprintf(stderr, "*** m2v_set_frame_size: %s\n", m2v_last_error(e));
                return 1;
            }
        }
        if (!pad && (xsize < 64 || xsize > (16 << XL) || xsize % 16)) {                        // TB:189-194
            printf("*** xsize=%4d is invalid, which must in range [64,%4d], and must be a multiple of 16\n", xsize, 16 << XL);
            return 1;
        }
        if (!pad && (ysize < 64 || ysize > (16 << YL) || ysize % 16)) {                        // TB:196-201
            printf("*** ysize=%4d is invalid, which must in range [64,%4d], and must be a multiple of 16\n", ysize, 16 << YL);
            return 1;
        }
        const int fw = ssw ? ssw : xsize, fh = ssw ? ssh : ysize;                              // the size of the file's frames
        const size_t fb = layout420 >= 0 ? (size_t)fw * fh + 2 * (size_t)((fw + 1) / 2) * (size_t)((fh + 1) / 2)
                                         : (size_t)fw * fh * (rgb >= M2V_RGB_RGBX32 && rgb <= M2V_RGB_XBGR32 ? 4 : 3);
        std::vector<uint8_t> frame(fb), word(1 << 20), es;
        size_t frames = 0, bytes = 0;
        const auto t0 = std::chrono::steady_clock::now();
        auto drain = [&](bool until_last) {
            for (;;) {
                int last = 0;
                long long n = m2v_pull(e, word.data(), word.size(), &last);
                if (n < 0) { fprintf(stderr, "*** m2v_pull: %s\n", m2v_last_error(e)); exit(1); }
                if (n) {
                    fwrite(word.data(), 1, (size_t)n, fo);
                    bytes += (size_t)n;
                    if (want_ps || want_ts || stats) es.insert(es.end(), word.begin(), word.begin() + n);
                }
                if (last || (!until_last && n == 0)) break;
                if (until_last && n == 0 && !m2v_busy(e)) break;
            }
        };
        if (resident) {
            // the detector runs in front of a chunk's plan on the resident entries: the file's complete frames go to device memory whole
            std::vector<uint8_t> all;
            while (fread(frame.data(), 1, fb, fi) == fb) { all.insert(all.end(), frame.begin(), frame.end()); ++frames; }
            const size_t cap = frames * ((size_t)xs16 * ys16 * 1216 + (size_t)ys16 * 8 + 64) + 256;
            void *d_in = nullptr, *d_out = nullptr, *d_rec = nullptr;
            size_t nb = 0;
            // a reconstructed frame is of the file's size: the coded size, or under -pad the size set
            const size_t rb = frames * ((size_t)xsize * ysize + 2 * (size_t)((xsize + 1) / 2) * (size_t)((ysize + 1) / 2));
            if (frames) {
                if (fr && (hipSetDevice(dev) != hipSuccess || hipMalloc(&d_rec, rb) != hipSuccess)) {
                    fprintf(stderr, "*** %zu bytes of device memory for the reconstruction: allocation failed\n", rb);
                    return 1;
                }
                if (fr && m2v_set_recon_out(e, d_rec, rb, reconfmt) < 0) { fprintf(stderr, "*** m2v_set_recon_out: %s\n", m2v_last_error(e)); return 1; }
                if (hipSetDevice(dev) != hipSuccess || hipMalloc(&d_in, all.size()) != hipSuccess || hipMalloc(&d_out, cap) != hipSuccess ||
                    hipMemcpy(d_in, all.data(), all.size(), hipMemcpyHostToDevice) != hipSuccess) {
                    fprintf(stderr, "*** staging %zu frames in device memory failed\n", frames);
                    return 1;
                }
                const int r = rgb >= 0 ? m2v_encode_resident_rgb(e, xs16, ys16, (uint32_t)pf, d_in, frames, rgb, matrix, d_out, cap, &nb, nullptr)
                            : layout420 >= 0 ? m2v_encode_resident420(e, xs16, ys16, (uint32_t)pf, d_in, frames, layout420, d_out, cap, &nb, nullptr)
                                             : m2v_encode_resident(e, xs16, ys16, (uint32_t)pf, d_in, frames, d_out, cap, &nb, nullptr);
                if (r < 0) { fprintf(stderr, "*** resident encode failed: %s\n", m2v_last_error(e)); return 1; }
                es.resize(nb);
                if (hipMemcpy(es.data(), d_out, nb, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "*** read-back failed\n"); return 1; }
                fwrite(es.data(), 1, nb, fo);
                bytes = nb;
                if (fr) {
                    std::vector<uint8_t> rec(rb);
                    if (hipMemcpy(rec.data(), d_rec, rb, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "*** read-back failed\n"); return 1; }
                    fwrite(rec.data(), 1, rb, fr);
                    m2v_set_recon_out(e, nullptr, 0, 0);
                    (void)hipFree(d_rec);
                    printf("  %s: %zu frames, %zu bytes\n", recon, frames, rb);
                }
                (void)hipFree(d_in);
                (void)hipFree(d_out);
            }
        }
        while (!resident && fread(frame.data(), 1, fb, fi) == fb) {                            // complete frames only (TB:220)
            printf("  start to encode video %d frame %3zu\n", num_video, frames);
            int r;
            if (rgb >= 0) {
                r = m2v_push_rgb(e, xs16, ys16, (uint32_t)pf, frame.data(), 1, rgb, matrix);
            } else if (layout420 >= 0) {
                r = m2v_push_frames420(e, xs16, ys16, (uint32_t)pf, frame.data(), 1, layout420);
            } else if (!bubbles) {
                r = m2v_push_frames(e, xs16, ys16, (uint32_t)pf, frame.data(), 1);
            } else {                                                                           // beat-level, odd batch sizes
                const size_t npix = (size_t)xsize * ysize;
                size_t b = 0, nb = npix / 4;
                r = 0;
                while (b < nb && r == 0) {
                    size_t take = 1 + (b * 7919) % 61;
                    if (take > nb - b) take = nb - b;
                    r = m2v_push_beats(e, xs16, ys16, (uint32_t)pf, frame.data() + b * 4,
                                       frame.data() + npix + b * 4, frame.data() + 2 * npix + b * 4, take, 0);
                    b += take;
                }
            }
            if (r < 0) { fprintf(stderr, "*** push failed: %s\n", m2v_last_error(e)); return 1; }
            ++frames;
            drain(false);
        }
        if (!resident) {
            if (m2v_sequence_stop(e) < 0) { fprintf(stderr, "*** stop failed: %s\n", m2v_last_error(e)); return 1; }
            drain(true);
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fclose(fi);
        fclose(fo);
        for (int kind = 0; kind < 2; ++kind) {
            if (!(kind ? want_ts : want_ps) || es.empty()) continue;
            size_t need = 0;
            int r = 0;
            std::vector<uint8_t> mux;
            if (devmux) {
                // the stream back in device memory, muxed there (a resident caller sets m2v_set_mux_out and never leaves the device)
                const uint64_t off = 0, nb = es.size();
                const size_t room = m2v_mux_bound(kind ? M2V_MUX_TS : M2V_MUX_PS, es.size(), frames);
                void *d_es = nullptr, *d_mux = nullptr;
                m2v_mux_stat rec{};
                if (hipSetDevice(dev) != hipSuccess || hipMalloc(&d_es, es.size()) != hipSuccess || hipMalloc(&d_mux, room) != hipSuccess ||
                    hipMemcpy(d_es, es.data(), es.size(), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "*** staging the stream in device memory failed\n"); return 1; }
                if (m2v_mux_device(e, kind ? M2V_MUX_TS : M2V_MUX_PS, d_es, &off, &nb, 1, d_mux, room, nullptr) < 0 || m2v_mux_report(e, &rec, 1) != 1) {
                    fprintf(stderr, "*** m2v_mux_device: %s\n", m2v_last_error(e));
                    return 1;
                }
                r = rec.status;
                need = (size_t)rec.out_bytes;
                mux.resize(need);
                if (r == 0 && hipMemcpy(mux.data(), d_mux, need, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "*** read-back failed\n"); return 1; }
                (void)hipFree(d_es);
                (void)hipFree(d_mux);
            } else {
                r = kind ? m2vc_mux_ts(es.data(), es.size(), nullptr, 0, &need) : m2vc_mux_ps(es.data(), es.size(), nullptr, 0, &need);
                mux.resize(need);
                if (r == 0) r = kind ? m2vc_mux_ts(es.data(), es.size(), mux.data(), mux.size(), &need)
                                     : m2vc_mux_ps(es.data(), es.size(), mux.data(), mux.size(), &need);
            }
            if (r < 0) { fprintf(stderr, "*** multiplexer failed (%d)\n", r); return 1; }
            const std::string name = std::string(out) + (kind ? ".ts" : ".mpg");
            FILE *fm = fopen(name.c_str(), "wb");
            if (!fm) { printf("*** couldn't open %s\n", name.c_str()); return 1; }
            fwrite(mux.data(), 1, need, fm);
            fclose(fm);
            printf("  %s: %zu bytes\n", name.c_str(), need);
        }
        if (stats) {
            std::vector<m2v_picture_stat> rec(frames);
            const long long got = m2v_picture_stats(e, rec.data(), rec.size());
            std::vector<m2vc_picture> pics(frames);
            size_t npics = 0;
            m2vc_stream_info info;
            if (got != (long long)frames || m2vc_scan(es.data(), es.size(), &info, pics.data(), pics.size(), &npics) < 0 || npics != frames) {
                fprintf(stderr, "*** statistics: %lld records, %zu pictures in the stream for %zu frames\n", got, npics, frames);
                return 1;
            }
            // samples of the measured region: the source's size (the coded size is the same without -pad)
            const double ny = (double)xsize * ysize, nc = (double)((xsize + 1) / 2) * ((ysize + 1) / 2);
            auto psnr = [](double sse, double n) { return sse > 0 ? 10.0 * std::log10(255.0 * 255.0 * n / sse) : INFINITY; };
            double sum[3] = {0, 0, 0}, low[3] = {INFINITY, INFINITY, INFINITY};
            unsigned long long bits = 0;
            for (size_t k = 0; k < frames; ++k) {
                const m2v_picture_stat &r = rec[k];
                const double db[3] = {psnr((double)r.sse[0], ny), psnr((double)r.sse[1], nc), psnr((double)r.sse[2], nc)};
                for (int c = 0; c < 3; ++c) { sum[c] += db[c]; if (db[c] < low[c]) low[c] = db[c]; }
                bits += r.mb_bits;
                printf("  stats video %d frame %3u %c  PSNR Y %6.2f U %6.2f V %6.2f  intra %5u inter %5u  mb bits %9llu  bytes %8llu\n", num_video, r.frame,
                       r.coding_type == 1 ? 'I' : 'P', db[0], db[1], db[2], r.intra_mbs, r.inter_mbs, (unsigned long long)r.mb_bits,
                       (unsigned long long)pics[k].bytes);
            }
            if (frames)
                printf("  stats video %d: mean PSNR Y %6.2f U %6.2f V %6.2f  min Y %6.2f U %6.2f V %6.2f  mb bits %llu\n", num_video, sum[0] / frames,
                       sum[1] / frames, sum[2] / frames, low[0], low[1], low[2], bits);
        }
        printf("end of video %d: %zu frames -> %zu bytes, %.3f s, %.1f MPixels/s incl. file I/O and PCIe\n", num_video, frames,
               bytes, s, (double)frames * xsize * ysize / s * 1e-6);
    }
    if (fr) fclose(fr);
    m2v_destroy(e);
    return 0;
}
