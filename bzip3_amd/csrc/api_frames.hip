// api_frames.hip -- the device-resident frame API of include/bz3_hip.h (plain, byte planes, delta, decoded sizes, and the partial decode calls:
// range, strided, select), its debug entry points and the batched CRC.  The only unit that includes frame.hpp and planes.hpp: their kernels are
// ordinary definitions.  The partial decode calls share one request form (Request), one list of gather segments with their side tables
// (GatherList) and one body (decompress_frames); what differs between them is how an entry point reads its parameters.  The two update calls
// share the same request form and front (request_front) and one body (update_frames), of which the sync call is a mode: its touched chunks are
// the ones a device comparison of the new tensor with the old one finds changed (diff_segments, planes.hpp k_diff_segments).
#include <functional>

#include "api_internal.hpp"
#include "frame.hpp"
#include "planes.hpp"

using namespace bz3;
using namespace bz3::api;

extern "C" {

// ---- device-resident frames (bz3_hip.h: bz3_hip_compress_device[_many] / bz3_hip_decompress_device[_many]) -------------------
// The frame API above with `in` and `out` in HBM of one GPU, for one frame or many in one call (the single-frame entry
// points are the n = 1 case).  A window of up to 256 blocks at a time, taken in frame order across frame boundaries: one
// state per block on the buffers' device and one slab of slots; every move between the caller's buffers and the slots is
// ONE launch of k_copy_segments (frame.hpp), frame and chunk headers travel as extra segments from a small staged buffer,
// and on decode the chunk headers of all frames are walked on the device (k_frame_walk_many, one lane per frame) and read
// back once per window.  The _planes entry points give every frame an element size: its blocks are split into byte planes on
// the way into their slots and merged on the way out (planes.hpp), in the same launches; elem_sizes == nullptr is 1 everywhere.
// The _delta entry points give a frame a base of the size of its input as well: a block's segment carries the address of the base bytes
// that pair with it, which the same launch subtracts before the split and adds after the merge; bases == nullptr is no base anywhere.
namespace {

// The device that owns `p` if it is device memory, else -1.  (The emulator's device memory is host memory, on device 0.)
int device_of(const void * p) {
    if (!p) return -1;
#ifdef BZ3_EMU
    return 0;
#else
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return a.type == hipMemoryTypeDevice ? a.device : -1;
#endif
}

constexpr size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// Device tables of one segment launch whose highest segment kind is `level` (planes.hpp SegLevel): the segments, then the nseg + 1 tile starts;
// from SEG_CLIP on, 16-byte aligned behind them, the [a, b) of every segment (two u64 each); from SEG_STRIDED on the STRIDED_PARAMS u64 of
// every segment behind the clips; with SEG_SELECT the SELECT_PARAMS u64 of every segment behind the periods.
constexpr size_t table_bytes(size_t nseg, int level) {
    size_t b = align16(nseg * sizeof(CopySeg)) + (nseg + 1) * sizeof(u32);
    if (level >= SEG_CLIP) b = align16(b) + nseg * 2 * sizeof(u64);
    if (level >= SEG_STRIDED) b += nseg * STRIDED_PARAMS * sizeof(u64);
    if (level >= SEG_SELECT) b += nseg * SELECT_PARAMS * sizeof(u64);
    return b;
}

// The last chunk byte a strided merge reads, c(nbytes - 1) for nbytes > 0, or UINT64_MAX where it does not fit 64 bits.
u64 strided_last_byte(u64 c0, u64 first, u64 run, u64 stride, u64 nbytes) {
    const u64 u = nbytes - 1;
    unsigned __int128 c = (unsigned __int128)c0 + u;
    if (u >= first) c += (unsigned __int128)((u - first) / run + 1) * (stride - run);
    return c > UINT64_MAX ? UINT64_MAX : (u64)c;
}

// A request's piece list as its walk and its gather want it (frame.hpp, planes.hpp): m + 1 pairs (s_j, P_j), the last one closing the table
// with P_m = L.  A request's table holds the pieces that are not empty, neighbours joined; a debug call's the list as it was given.
struct PieceTable {
    std::vector<u64> tab;
    u64 m = 0, L = 0;
    u64 given_end = 0;  // s + l of the last piece of the list as it was given (empty or not), 0 for no piece: what bz3_hip.h's checks speak of
    u64 s(u64 j) const { return tab[2 * j]; }
    u64 P(u64 j) const { return tab[2 * j + 1]; }
    u64 l(u64 j) const { return P(j + 1) - P(j); }
    u64 last_end() const { return m ? s(m - 1) + l(m - 1) : 0; }
    // `pieces`: m_in pairs (s_j, l_j).  False for a list that bz3_hip.h calls invalid.  join == false: every piece is kept as it is.
    bool take(const u64 * pieces, u64 m_in, bool join = true) {
        tab.clear();
        m = L = given_end = 0;
        if (m_in && !pieces) return false;
        u64 end = 0, kept_end = 0;  // of the piece before, of the last piece kept
        for (u64 j = 0; j < m_in; j++) {
            const u64 sj = pieces[2 * j], lj = pieces[2 * j + 1];
            if (sj + lj < sj || (j && sj < end)) return false;
            if (join && lj && m && sj == kept_end) {
                L += lj;  // joins the piece before it
            } else if (lj || !join) {
                tab.push_back(sj);
                tab.push_back(L);
                L += lj;
                m++;
            }
            if (L < lj) return false;  // (count * L would not fit either)
            end = sj + lj;
            if (lj) kept_end = end;
        }
        given_end = end;
        tab.push_back(0);
        tab.push_back(L);
        return true;
    }
    // The wanted bytes of a period below its byte r.
    u64 below(u64 r) const {
        const u32 j = first_piece_behind(tab.data(), (u32)m, r);
        return j == m ? L : P(j) + (r > s(j) ? r - s(j) : 0);
    }
    // The byte of a period that is its wanted byte r < L.
    u64 byte(u64 r) const {
        const u64 j = piece_of(tab.data(), (u32)m, r);
        return s(j) + (r - P(j));
    }
};

// The segments of one launch.  A segment of a partial merge (planes.hpp: clipped, strided, select) carries the row of its kind's side table with
// it, so a segment and its parameters cannot fall out of step; copy_segments lays the tables out.  `level` is the highest kind among the
// segments: it alone decides which tables are uploaded and which kernel runs.
struct GatherList {
    struct Entry {
        CopySeg seg;
        u64 row[SELECT_PARAMS];  // of the side table that seg.mode names: [a, b), STRIDED_PARAMS or SELECT_PARAMS
    };
    std::vector<Entry> v;
    int level = SEG_DELTA;
    bool patched = false;  // the list holds a clipped or a select split: the launch is k_patch_segments or k_patch_select_segments, and holds no partial merge
    bool merged = false;   // the list holds a partial merge
    bool replaned = false;  // the list holds a replane segment: the launch is k_replane_segments, and holds no select split
    size_t size() const { return v.size(); }
    void clear() {
        v.clear();
        level = SEG_DELTA;
        patched = merged = replaned = false;
    }
    // A segment as it is: a copy, a split, a merge, with or without a base.
    void plain(const CopySeg & sg) { v.push_back({sg, {}}); }
    // The chunk bytes [a, b) of a decoded chunk of s bytes in `slot`, element size k, to dst (and base, or 0), which address the clip's first
    // byte: a whole chunk and every k = 1 clip are ordinary segments, the rest clipped merges.
    void range(u64 slot, u64 s, u64 k, u64 a, u64 b, u64 dst, u64 base) {
        if (k <= 1 || a == b || (a == 0 && b == s)) return plain({slot + (k <= 1 ? a : 0), dst, b - a, k | PLANES_INVERSE, base});
        v.push_back({{slot, dst, s, k | PLANES_INVERSE | PLANES_CLIP, base}, {a, b}});
        level = std::max<int>(level, SEG_CLIP);
        merged = true;
    }
    // The write mirror of range(): the chunk bytes [a, b) of the chunk of s bytes that `slot` holds in split form get the new values src[0, b - a)
    // (less base[0, b - a), or 0), which address the clip's first byte.  A whole chunk and every k = 1 clip are ordinary segments, the rest clipped
    // splits (planes.hpp, "Clipped split").
    void patch(u64 src, u64 base, u64 slot, u64 s, u64 k, u64 a, u64 b) {
        if (k <= 1 || a == b || (a == 0 && b == s)) return plain({src, slot + (k <= 1 ? a : 0), b - a, k, base});
        v.push_back({{src, slot, s, k | PLANES_CLIP, base}, {a, b}});
        level = std::max<int>(level, SEG_CLIP);
        patched = true;
    }
    // The kept head of a resized chunk: the chunk bytes [0, a) of the decoded chunk of s_old bytes that `src` holds in split form, to where `slot`,
    // which is to hold the split form of a chunk of s_new bytes, keeps them (planes.hpp, "Replane"); a <= min(s_old, s_new).  k = 1 is a plain copy,
    // and nothing where the chunk was decoded into `slot` itself.
    void replane(u64 src, u64 slot, u64 s_old, u64 s_new, u64 k, u64 a) {
        if (a == 0 || (k <= 1 && src == slot)) return;
        if (k <= 1) return plain({src, slot, a, 0, 0});
        v.push_back({{src, slot, s_new, k | PLANES_REPLANE, 0}, {s_old, a}});
        level = std::max<int>(level, SEG_CLIP);
        patched = replaned = true;
    }
    // The same for a chunk of which a strided range wants the nbytes bytes c(u) (planes.hpp, "Strided merge"; first in [1, run], stride >= run):
    // a share within one run (nbytes <= first) is the clipped or whole segment above, anything else a strided merge.
    void strided(u64 slot, u64 s, u64 k, u64 c0, u64 first, u64 run, u64 stride, u64 nbytes, u64 dst, u64 base) {
        if (nbytes <= first) return range(slot, s, k, c0, c0 + nbytes, dst, base);
        v.push_back({{slot, dst, s, k | PLANES_INVERSE | PLANES_STRIDED, base}, {c0, first, run, stride, nbytes}});
        level = std::max<int>(level, SEG_STRIDED);
        merged = true;
    }
    // The same for a chunk of which a select request wants the nbytes > 0 bytes c(u) (planes.hpp, "Select merge": rel, stride, q0, r0 < L, the
    // table t at device address d_tab): a share within one piece is the clipped or whole segment above, anything else a select merge.
    void select(u64 slot, u64 s, u64 k, u64 rel, u64 stride, const PieceTable & t, u64 d_tab, u64 q0, u64 r0, u64 nbytes, u64 dst, u64 base) {
        const u64 j = piece_of(t.tab.data(), (u32)t.m, r0);
        if (nbytes <= t.P(j + 1) - r0) {
            const u64 c0 = rel + q0 * stride + t.s(j) + (r0 - t.P(j));
            return range(slot, s, k, c0, c0 + nbytes, dst, base);
        }
        v.push_back({{slot, dst, s, k | PLANES_INVERSE | PLANES_SELECT, base}, {rel, stride, q0, r0, nbytes, d_tab, t.m}});
        level = SEG_SELECT;
        merged = true;
    }
    // The write mirror of select(): the chunk bytes c(u), u < nbytes (nbytes > 0), of the chunk of s bytes that `slot` holds in split form get the
    // new values src[0, nbytes) (less base[0, nbytes), or 0).  A share within one piece is the clipped or whole split of patch(), anything else a
    // select split (planes.hpp, "Select split").
    void patch_select(u64 src, u64 base, u64 slot, u64 s, u64 k, u64 rel, u64 stride, const PieceTable & t, u64 d_tab, u64 q0, u64 r0, u64 nbytes) {
        const u64 j = piece_of(t.tab.data(), (u32)t.m, r0);
        if (nbytes <= t.P(j + 1) - r0) {
            const u64 c0 = rel + q0 * stride + t.s(j) + (r0 - t.P(j));
            return patch(src, base, slot, s, k, c0, c0 + nbytes);
        }
        v.push_back({{src, slot, s, k | PLANES_SELECT, base}, {rel, stride, q0, r0, nbytes, d_tab, t.m}});
        level = SEG_SELECT;
        patched = true;
    }
};

// Copies the segments of g (absolute device addresses) in one launch on stream s; d_tab holds table_bytes(g.size(), g.level) bytes.  The kernel
// is k_patch_segments for a list with a clipped split (k_patch_select_segments where it holds a select split as well, k_replane_segments where it holds a replane segment), else the one of g.level; at SEG_DELTA k_delta_segments where a segment has a base, else k_move_segments where one has an element size, else
// k_copy_segments (planes.hpp).  The caller synchronises (the host tables are staged from pageable memory and must outlive the copy).
void copy_segments(const GatherList & g, std::vector<u8> & staging, u8 * d_tab, hipStream_t s) {
    const size_t n = g.size(), bytes = table_bytes(n, g.level), seg_bytes = align16(n * sizeof(CopySeg));
    const size_t clip_off = table_bytes(n, SEG_CLIP) - n * 2 * sizeof(u64), period_off = table_bytes(n, SEG_CLIP), select_off = table_bytes(n, SEG_STRIDED);
    staging.assign(bytes, 0);
    u32 * starts = (u32 *)(staging.data() + seg_bytes);
    u64 tiles = 0;
    bool planes = false, delta = false;
    for (size_t i = 0; i < n; i++) {
        const CopySeg & sg = g.v[i].seg;
        const u64 * row = g.v[i].row;
        const u64 k = sg.mode & 0xff;
        memcpy(staging.data() + i * sizeof(CopySeg), &sg, sizeof(CopySeg));
        starts[i] = (u32)tiles;
        if (sg.mode & PLANES_SELECT) {  // (a segment of a kind raised g.level to it: its table lies inside `bytes`)
            memcpy(staging.data() + select_off + i * SELECT_PARAMS * sizeof(u64), row, SELECT_PARAMS * sizeof(u64));
            tiles += strided_tiles(row[4], k);
        } else if (sg.mode & PLANES_STRIDED) {
            memcpy(staging.data() + period_off + i * STRIDED_PARAMS * sizeof(u64), row, STRIDED_PARAMS * sizeof(u64));
            tiles += strided_tiles(row[4], k);
        } else if (sg.mode & PLANES_CLIP) {
            memcpy(staging.data() + clip_off + i * 2 * sizeof(u64), row, 2 * sizeof(u64));
            tiles += clip_tiles(sg.len, k, row[0], row[1]);
        } else if (sg.mode & PLANES_REPLANE) {  // (its row, len_old and a, lies in the clip table)
            memcpy(staging.data() + clip_off + i * 2 * sizeof(u64), row, 2 * sizeof(u64));
            tiles += replane_tiles(row[1], k);
        } else {
            tiles += segment_tiles(sg);
        }
        planes |= k > 1;
        delta |= sg.base != 0;
    }
    if (g.patched && g.merged) throw std::logic_error("patch segments and partial merges in one launch");
    if (g.replaned && g.level == SEG_SELECT) throw std::logic_error("a replane segment and a select split in one launch");
    if (tiles >= ((u64)1 << 24)) throw std::length_error("segment copy larger than 256 GiB");
    starts[n] = (u32)tiles;
    if (!tiles) return;
    HIP_CHECK(hipMemcpyAsync(d_tab, staging.data(), bytes, hipMemcpyHostToDevice, s));
    const dim3 grid((u32)tiles), block(COPY_THREADS);
    const CopySeg * d_segs = (const CopySeg *)d_tab;
    const u32 * d_starts = (const u32 *)(d_tab + seg_bytes);
    const u64 * d_clips = (const u64 *)(d_tab + clip_off);
    const u64 * d_periods = (const u64 *)(d_tab + period_off);
    const u64 * d_selects = (const u64 *)(d_tab + select_off);
    if (g.replaned) launch(k_replane_segments, grid, block, 0, s, d_segs, d_starts, (u32)n, d_clips);
    else if (g.patched && g.level == SEG_SELECT) launch(k_patch_select_segments, grid, block, 0, s, d_segs, d_starts, (u32)n, d_clips, d_selects);
    else if (g.patched) launch(k_patch_segments, grid, block, 0, s, d_segs, d_starts, (u32)n, d_clips);
    else if (g.level == SEG_SELECT) launch(k_select_segments, grid, block, 0, s, d_segs, d_starts, (u32)n, d_clips, d_periods, d_selects);
    else if (g.level == SEG_STRIDED) launch(k_strided_segments, grid, block, 0, s, d_segs, d_starts, (u32)n, d_clips, d_periods);
    else if (g.level == SEG_CLIP) launch(k_range_segments, grid, block, 0, s, d_segs, d_starts, (u32)n, d_clips);
    else launch(delta ? k_delta_segments : planes ? k_move_segments : k_copy_segments, grid, block, 0, s, d_segs, d_starts, (u32)n);
}

// Compares the diff segments of v (planes.hpp: src and base the two runs, mode the index of the segment's flag) in one launch of k_diff_segments on
// stream s and reads the flags back: flags[j], j < nflags, is 1 where a segment with mode == j differs and 0 otherwise.  d_tab holds
// table_bytes(v.size(), SEG_DELTA) bytes, d_flags nflags u32.  Complete on return; nothing is launched for a list without a byte.
void diff_segments(const std::vector<CopySeg> & v, std::vector<u8> & staging, u8 * d_tab, u32 * d_flags, u32 * flags, size_t nflags, hipStream_t s) {
    const size_t n = v.size(), seg_bytes = align16(n * sizeof(CopySeg));
    staging.assign(table_bytes(n, SEG_DELTA), 0);
    u32 * starts = (u32 *)(staging.data() + seg_bytes);
    u64 tiles = 0;
    for (size_t i = 0; i < n; i++) {
        if (v[i].mode >= nflags) throw std::logic_error("diff flag out of range");
        memcpy(staging.data() + i * sizeof(CopySeg), &v[i], sizeof(CopySeg));
        starts[i] = (u32)tiles;
        tiles += copy_tiles(v[i].src, v[i].len);
        if (tiles >= ((u64)1 << 24)) throw std::length_error("segment diff larger than 256 GiB");
    }
    std::fill(flags, flags + nflags, 0u);
    if (!tiles) return;
    starts[n] = (u32)tiles;
    HIP_CHECK(hipMemcpyAsync(d_tab, staging.data(), staging.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_flags, 0, nflags * sizeof(u32), s));
    launch(k_diff_segments, dim3((u32)tiles), dim3(COPY_THREADS), 0, s, (const CopySeg *)d_tab, (const u32 *)(d_tab + seg_bytes), (u32)n, d_flags);
    HIP_CHECK(hipMemcpyAsync(flags, d_flags, nflags * sizeof(u32), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

constexpr size_t FRAME_WINDOW_MAX = 256;  // blocks per window: one CU per block during the CM stage (the host frame path's rule)
constexpr size_t WALK_RECORDS = 4096;     // chunk records of one walk (bz3_hip_frame_decoded_sizes_device; a window's walk takes at most FRAME_WINDOW_MAX)
static_assert(WALK_RECORDS >= FRAME_WINDOW_MAX, "a window's walk must fit the records");

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Layout of a call's small device buffer, sized for its n frames: staged headers (one 13-byte frame header per frame and one
// 8-byte chunk header per block of a window at most), the copy tables of a window (two segments per block, one per frame
// header; with room for their clips and periods), the walk's arguments, records and tails.  A call that walks with piece tables
// (piece_bytes > 0 of them, uploaded once per call) has them behind the tails and room for the piece-list parameters in its copy tables;
// every other call has the layout and the size it had.  An update (update_frames) packs up to two runs of verbatim bytes per frame beside the two
// segments of every block, the frame header travelling in the first run: `runs` = 2 segments per frame instead of 1.  A sync (update_frames with
// `olds`) has behind all that the diff table of a walk round, one segment per record, and the round's flags: `diff_segs` = WALK_RECORDS.
struct MetaLayout {
    size_t n = 0, segs = 0, hdr = 0, tab = 0, args = 0, rec = 0, tails = 0, pieces = 0, diff = 0, flags = 0, bytes = 0;
    MetaLayout() = default;
    explicit MetaLayout(size_t frames, size_t piece_bytes = 0, size_t runs = 1, size_t diff_segs = 0) : n(frames), segs(2 * FRAME_WINDOW_MAX + runs * frames) {
        tab = align256(13 * n + 8 * FRAME_WINDOW_MAX);
        args = tab + align256(table_bytes(segs, piece_bytes ? SEG_SELECT : SEG_STRIDED));
        rec = args + align256(n * sizeof(WalkArg));
        tails = rec + align256(WALK_RECORDS * sizeof(WalkChunk));
        pieces = tails + align256(n * sizeof(WalkTail));
        diff = pieces + align256(piece_bytes);
        flags = diff + (diff_segs ? align256(table_bytes(diff_segs, SEG_DELTA)) : 0);
        bytes = flags + align256(diff_segs * sizeof(u32));
    }
};

// Blocks per window: FRAME_WINDOW_MAX, or fewer under BZ3_HIP_FRAME_WINDOW (tests: windows that cut through frames).
size_t frame_window_limit() {
    size_t limit = FRAME_WINDOW_MAX;
    if (const char * e = getenv("BZ3_HIP_FRAME_WINDOW"))
        if (atoi(e) > 0 && (size_t)atoi(e) < limit) limit = (size_t)atoi(e);
    return limit;
}

// The device, stream, states, slab and small buffer of one call over n frames.
struct DeviceFrames {
    int device = -1;
    hipStream_t s = nullptr;  // the lead state's stream (its own for the walks before the states exist)
    bool own_stream = false;
    u8 * meta = nullptr;
    MetaLayout lay;
    u8 * slab = nullptr;
    size_t stride = 0;
    std::vector<bz3_state *> states;
    GatherList gather;  // the segments of the next launch
    std::vector<u8> staging;
    ~DeviceFrames() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (s) (void)hipStreamSynchronize(s);
        for (bz3_state * st : states) state_release(st);
        if (slab) (void)hipFree(slab);
        if (meta) (void)hipFree(meta);
        if (own_stream && s) (void)hipStreamDestroy(s);
    }
    bool open(int dev, size_t n, size_t piece_bytes = 0, size_t runs = 1, size_t diff_segs = 0) {  // the device, a stream and the small buffer
        if (dev < 0 || dev >= device_count() || !get_ctx(dev)) return false;
        device = dev;
        lay = MetaLayout(n, piece_bytes, runs, diff_segs);
        HIP_CHECK(hipSetDevice(dev));
        HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        own_stream = true;
        HIP_CHECK(hipMalloc((void **)&meta, lay.bytes));
        return true;
    }
    // Up to `want` states of block_size (the call's largest) on the device and a slab of as many slots, within the memory the
    // headroom rule leaves; at least one or false.
    bool init(u32 block_size, size_t want) {
        size_t limit = frame_window_limit();
        const size_t cap = (bz3_bound(block_size) + 4096 + 255) & ~(size_t)255;  // a state's cap (new_state_on)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            // per block: a slot and a swap buffer (owned or borrowed); beside them the headroom, the stages' workspace and two LZP contexts
            const size_t fixed = ws_headroom() + workspace_bytes_for((u64)block_size + 64) + 2 * lzp_encode_ctx_bytes((u64)block_size + 128) + ((size_t)64 << 20);
            const size_t by_mem = free_b > fixed ? (free_b - fixed) / (2 * cap) : 0;
            if (by_mem < limit) limit = by_mem;
        }
        if (want > limit) want = limit;
        if (want < 1) want = 1;
        for (size_t i = 0; i < want; i++) {
            bz3_state * st = new_state_on((int32_t)block_size, device);
            if (!st) break;
            states.push_back(st);
        }
        while (!states.empty()) {
            if (hipMalloc((void **)&slab, states.size() * cap) == hipSuccess) break;
            (void)hipGetLastError();
            slab = nullptr;
            const size_t keep = states.size() / 2;
            while (states.size() > keep) {
                state_release(states.back());
                states.pop_back();
            }
        }
        if (states.empty()) return false;
        stride = cap;
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipStreamDestroy(s));
        own_stream = false;
        s = states[0]->stream;
        return true;
    }
    u8 * slot(size_t k) const { return slab + k * stride; }
    void copy() {  // the segments collected in `gather`, one launch, complete on return
        if (gather.size() > lay.segs) throw std::length_error("copy table overflow");
        copy_segments(gather, staging, meta + lay.tab, s);
        HIP_CHECK(hipStreamSynchronize(s));
        gather.clear();
    }
    void stage_headers(const std::vector<u8> & h) {
        if (h.size() > lay.tab - lay.hdr) throw std::length_error("staged header overflow");
        if (!h.empty()) HIP_CHECK(hipMemcpyAsync(meta + lay.hdr, h.data(), h.size(), hipMemcpyHostToDevice, s));
    }
    // The piece tables of a call, one after the other: one upload per call.  Returns the device address of the first.
    u64 upload_pieces(const std::vector<u64> & tables) {
        if (!tables.empty()) {
            HIP_CHECK(hipMemcpyAsync(meta + lay.pieces, tables.data(), tables.size() * sizeof(u64), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        return (u64)(meta + lay.pieces);
    }
    // One launch of k_frame_walk_many over args.size() frames and one read-back: tails[q] is frame q's resume state, its
    // records are rec[args[q].rec_base ..].
    void walk(const std::vector<WalkArg> & args, std::vector<WalkChunk> & rec, std::vector<WalkTail> & tails) {
        const size_t n = args.size();
        size_t nrec = 0;
        for (const WalkArg & a : args) nrec = std::max(nrec, (size_t)a.rec_base + a.limit);
        if (n > lay.n || nrec > WALK_RECORDS) throw std::length_error("walk larger than its buffer");
        tails.resize(n);
        rec.resize(nrec);
        if (!n) return;
        HIP_CHECK(hipMemcpyAsync(meta + lay.args, args.data(), n * sizeof(WalkArg), hipMemcpyHostToDevice, s));
        bool period = false, select = false;
        for (const WalkArg & a : args) period |= a.count > 1, select |= a.m > 0;
        launch(select ? k_frame_walk_select : period ? k_frame_walk_strided : k_frame_walk_many, dim3((u32)((n + WALK_THREADS - 1) / WALK_THREADS)), dim3(WALK_THREADS), 0, s,
               (const WalkArg *)(meta + lay.args), (u32)n, (WalkChunk *)(meta + lay.rec), (WalkTail *)(meta + lay.tails));
        if (nrec) HIP_CHECK(hipMemcpyAsync(rec.data(), meta + lay.rec, nrec * sizeof(WalkChunk), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(tails.data(), meta + lay.tails, n * sizeof(WalkTail), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
};

// Where a frame's walk stands: (off, planned, done) resume it; off == 0 before its header was read.
struct WalkPos {
    u64 off = 0, planned = 0;
    u32 done = 0, block_size = 0, n_blocks = 0;
    WalkArg arg(const u8 * in, size_t in_size, size_t buf_max, u32 limit, u32 rec_base) const {
        return WalkArg{(u64)in, (u64)in_size, (u64)buf_max, off, planned, done, limit, rec_base, block_size, n_blocks, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
    // the chunks that hold a byte of [lo, hi); with count > 1, of the `count` runs of `run` bytes that start `stride` apart from lo on
    // with m > 0, of the `count` periods `stride` apart from lo on, the m pieces of the table at device address `pieces`
    WalkArg range_arg(const u8 * in, size_t in_size, u64 lo, u64 hi, u32 limit, u32 rec_base, u64 run = 0, u64 stride = 0, u64 count = 0, u64 pieces = 0, u32 m = 0) const {
        return WalkArg{(u64)in, (u64)in_size, (u64)SIZE_MAX, off, planned, done, limit, rec_base, block_size, n_blocks, 1, lo, hi, run, stride, count, pieces, m, 0};
    }
    void take(const WalkTail & t) {
        off = t.off;
        planned = t.planned;
        done = t.done;
        block_size = t.block_size;
        n_blocks = t.n_blocks;
    }
};

// The frame headers of the frames with live[i]: one walk with limit 0.  A frame with a bad header gets its code in rcs and
// leaves `live`.
void walk_frame_headers(DeviceFrames & f, s32 n, const u8 * const * ins, const size_t * in_sizes, std::vector<WalkPos> & pos, std::vector<char> & live, int * rcs) {
    std::vector<WalkArg> args;
    std::vector<s32> who;
    for (s32 i = 0; i < n; i++)
        if (live[i]) {
            args.push_back(pos[i].arg(ins[i], in_sizes[i], SIZE_MAX, 0, 0));
            who.push_back(i);
        }
    std::vector<WalkChunk> rec;
    std::vector<WalkTail> tails;
    f.walk(args, rec, tails);
    for (size_t q = 0; q < who.size(); q++) {
        const s32 i = who[q];
        if (tails[q].err != BZ3_OK) {
            rcs[i] = tails[q].err;
            live[i] = 0;
        } else {
            pos[i].take(tails[q]);
        }
    }
}

// The buffers of a call's walks over its chunk headers, and one round of plain walks: args[q] walks frame who[q], whose records are
// rec[args[q].rec_base ..] and whose resume state is tails[q].
struct WalkRound {
    std::vector<WalkArg> args;
    std::vector<s32> who;
    std::vector<WalkChunk> rec;
    std::vector<WalkTail> tails;
    // Plans and runs a round over the frames i of [from, n) with want(i) that have a chunk left, in order: a frame's limit is what is left of it or
    // of the `budget` of records, its capacity buf_max(i).  One launch and one read-back; false, and neither, where no such frame is left.
    bool plain(DeviceFrames & f, const std::vector<WalkPos> & pos, const u8 * const * ins, const size_t * in_sizes, s32 from, s32 n, u32 budget,
               const std::function<bool(s32)> & want, const std::function<size_t(s32)> & buf_max) {
        args.clear();
        who.clear();
        u32 base = 0;
        for (s32 i = from; i < n && budget; i++) {
            if (!want(i) || pos[i].done == pos[i].n_blocks) continue;
            const u32 lim = std::min(pos[i].n_blocks - pos[i].done, budget);
            args.push_back(pos[i].arg(ins[i], in_sizes[i], buf_max(i), lim, base));
            who.push_back(i);
            base += lim;
            budget -= lim;
        }
        if (args.empty()) return false;
        f.walk(args, rec, tails);
        return true;
    }
};

// ---- compress: n frames whose buffers passed the pointer checks, on device dev --------------------------------------------
// Blocks go through windows in frame order, across frame boundaries: scatter (one copy launch), run_encode (one CM launch
// for the window's blocks of all frames), pack (the frame headers of the frames that start in the window, the chunk headers
// and the coded slots: one copy launch).  Every frame keeps its own output position and error.
// bases (or nullptr): per frame nullptr, or in_sizes[i] bytes the frame is coded against; block j pairs with base bytes [j bs, j bs + len_j).
void compress_frames(int dev, u32 block_size_arg, s32 n, const u32 * elem_sizes, const u8 * const * ins, const u8 * const * bases, const size_t * in_sizes,
                     u8 * const * outs, size_t * out_sizes, int * rcs) {
    struct Frame {
        u32 bs = 0, nb = 0, next = 0;  // effective block size, blocks, next block to scatter
        size_t pos = 0, buf_max = 0;   // bytes written, capacity
        bool live = false, started = false, fin = false;
    };
    std::vector<Frame> fr((size_t)n);
    u32 bs_max = 0;
    u64 total = 0;
    for (s32 i = 0; i < n; i++) {
        rcs[i] = BZ3_OK;
        Frame & x = fr[i];
        const size_t in_size = in_sizes[i];
        u32 bs = block_size_arg;
        if (bs > in_size) bs = (u32)bz3_bound(in_size);  // :877
        x.bs = bs <= (u32)KiB65 ? (u32)KiB65 : bs;
        x.nb = (u32)(in_size / x.bs);
        if (in_size % x.bs) x.nb++;
        if (x.bs > (u32)MiB511) {  // :879-886 (bz3_new)
            rcs[i] = BZ3_ERR_INIT;
            continue;
        }
        x.live = true;
        bs_max = std::max(bs_max, x.bs);
        total += x.nb;
    }
    if (!bs_max) return;
    DeviceFrames f;
    bool ok = false;
    try {
        ok = f.open(dev, (size_t)n) && f.init(bs_max, (size_t)std::min<u64>(total, FRAME_WINDOW_MAX));
    } catch (...) {
        ok = false;
    }
    for (s32 i = 0; i < n; i++) {
        Frame & x = fr[i];
        if (!x.live) continue;
        if (!ok) {
            rcs[i] = BZ3_ERR_INIT;
            x.live = false;
            continue;
        }
        x.buf_max = out_sizes[i];
        out_sizes[i] = 0;
        if (x.buf_max < 13 || x.buf_max < bz3_bound(in_sizes[i])) {  // (bz3_bound(in_size) covers the frame, so no chunk overflows it later)
            rcs[i] = BZ3_ERR_DATA_TOO_BIG;
            x.live = false;
        }
    }
    if (!ok) return;
    try {
        DeviceGuard g(dev);
        const u32 W = (u32)f.states.size();
        std::vector<s32> sizes(W), orig(W), owner(W);
        std::vector<void *> slots(W);
        std::vector<s32> heads, touched;
        std::vector<u8> hdr;
        s32 cur = 0;  // frames before it are finished
        for (;;) {
            while (cur < n && (!fr[cur].live || fr[cur].fin)) cur++;
            if (cur == n) break;
            // scatter: the next W blocks in frame order, block k to slot k
            u32 cnt = 0;
            heads.clear();
            touched.clear();
            for (s32 i = cur; i < n && cnt < W; i++) {
                Frame & x = fr[i];
                if (!x.live || x.fin) continue;
                if (!x.started) heads.push_back(i);
                touched.push_back(i);
                for (; x.next < x.nb && cnt < W; x.next++, cnt++) {
                    s32 size = (s32)x.bs;
                    if (x.next == x.nb - 1) size = (s32)(in_sizes[i] % x.bs);  // (sic) :914 -- 0 when in_size is a multiple
                    sizes[cnt] = orig[cnt] = size;
                    owner[cnt] = i;
                    slots[cnt] = f.slot(cnt);
                    f.states[cnt]->block_size = (s32)x.bs;  // every check of the block is made against its own frame's block size
                    f.states[cnt]->last_error = BZ3_OK;
                    f.gather.plain({(u64)(ins[i] + (size_t)x.next * x.bs), (u64)f.slot(cnt), (u64)size, elem_sizes ? (u64)elem_sizes[i] : 0,
                                      bases && bases[i] ? (u64)(bases[i] + (size_t)x.next * x.bs) : 0});
                }
            }
            if (cnt) {
                f.copy();
                run_encode(f.states.data(), slots.data(), sizes.data(), (s32)cnt, false);
            }
            // pack: frame headers, chunk headers from the staged buffer, the coded slots behind them
            hdr.clear();
            for (s32 i : heads) {
                Frame & x = fr[i];
                const size_t h = hdr.size();
                hdr.insert(hdr.end(), {'B', 'Z', '3', 'v', '1'});
                hdr.resize(h + 13);
                wr_le32(hdr.data() + h + 5, x.bs);
                wr_le32(hdr.data() + h + 9, x.nb);
                f.gather.plain({(u64)(f.meta + f.lay.hdr + h), (u64)outs[i], 13});
                x.pos = 13;
                x.started = true;
            }
            for (u32 k = 0; k < cnt; k++) {
                const s32 i = owner[k];
                Frame & x = fr[i];
                if (!x.live) continue;  // an earlier block of its frame failed in this window
                if (bz3_last_error(f.states[k]) != BZ3_OK) {  // :917-922
                    rcs[i] = f.states[k]->last_error;
                    x.live = false;
                    continue;
                }
                const s32 osz = sizes[k];
                if (osz < 0 || x.pos + 8 + (size_t)osz > x.buf_max) {  // (never taken: bz3_bound(in_size) covers the frame)
                    rcs[i] = BZ3_ERR_DATA_TOO_BIG;
                    x.live = false;
                    continue;
                }
                const size_t h = hdr.size();
                hdr.resize(h + 8);
                wr_le32(hdr.data() + h, (u32)osz);
                wr_le32(hdr.data() + h + 4, (u32)orig[k]);
                f.gather.plain({(u64)(f.meta + f.lay.hdr + h), (u64)(outs[i] + x.pos), 8});
                f.gather.plain({(u64)f.slot(k), (u64)(outs[i] + x.pos + 8), (u64)osz});
                x.pos += (size_t)osz + 8;
            }
            f.stage_headers(hdr);
            f.copy();
            for (s32 i : touched) {
                out_sizes[i] = fr[i].pos;
                fr[i].fin = fr[i].live && fr[i].next == fr[i].nb;
            }
        }
    } catch (const HipError & e) {
        fprintf(stderr, "bzip3_amd: HIP failure '%s' at %s:%d\n", e.what, e.file, e.line);
        for (s32 i = 0; i < n; i++)
            if (fr[i].live && !fr[i].fin) rcs[i] = BZ3_ERR_BWT;
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (fr[i].live && !fr[i].fin) rcs[i] = BZ3_ERR_BWT;
    }
}

// What a partial decode call wants of one frame: the first w bytes of the bytes phi(t) of bz3_hip.h, in its normal form.  The three calls name
// them differently and each reduces to the form below it wherever it can, so that a request the lower call could have made takes that call's path:
//   range    phi(t) = lo + t                                                        count == 0
//   strided  phi(t) = lo + (t / run) stride + t % run                               count > 1 runs, stride != run
//   select   phi(t) = lo + (t / L) stride + s_j + (t % L - P_j), piece j of `sel`   count >= 1 periods, two or more pieces
// cut() fixes w at the smallest of *out_size, the base's size and what the request names, and then normalises: a strided request of one run (after
// the cut) or with stride == run is the range (lo, w); a select request with w <= l_0 is the range (lo + s_0, w), any other one has `count` cut
// to the periods w reaches.  (An entry point has already turned a piece list that joins to one piece into its strided request, and one without
// a byte into the empty one.)
struct Request {
    u64 lo = 0, wanted = UINT64_MAX;     // phi(0); the bytes the request names
    u64 run = 0, stride = 0, count = 0;  // count periods `stride` apart, of each its first `run` bytes ...
    const PieceTable * sel = nullptr;    // ... or the L bytes of the pieces of this table, which the device has at d_tab
    u64 d_tab = 0;
    u64 w = 0, hi = 0;                   // after cut(): the bytes wanted, and end() = phi(w - 1) + 1: no chunk from there on is needed
    static Request range(u64 offset) {
        Request r;
        r.lo = offset;
        return r;
    }
    static Request strided(u64 offset, u64 run, u64 stride, u64 count) {  // (count run fits 64 bits: the caller's check)
        Request r = range(offset);
        r.wanted = count * run, r.run = run, r.stride = stride, r.count = count;
        return r;
    }
    static Request select(u64 offset, u64 stride, u64 count, const PieceTable & t) {  // (count L fits 64 bits)
        if (t.L == 0 || count == 0) return strided(offset, 0, 0, 0);
        if (t.m == 1) return strided(offset + t.s(0), t.L, stride, count);
        Request r = strided(offset, t.L, stride, count);
        r.sel = &t;
        return r;
    }
    void cut(u64 cap) {
        w = std::min(cap, wanted);
        const u64 periods = w && count ? (w - 1) / run + 1 : 0;  // (w > 0 with count > 0: run > 0)
        if (sel && w > sel->l(0)) {
            count = periods;
            if (count == 1) stride = std::max(stride, sel->last_end());  // (one period: its stride is never used, and may be 0)
        } else if (!sel && periods > 1 && stride != run) {
            count = periods;
        } else {
            if (sel && w) lo += sel->s(0);
            sel = nullptr;
            run = stride = count = 0;
        }
        hi = end();
    }
    u64 end() const {
        if (!count) return lo + w < lo ? UINT64_MAX : lo + w;
        const u64 r = (w - 1) - (count - 1) * run;  // the last byte's place among its period's wanted bytes
        return lo + (count - 1) * stride + (sel ? sel->byte(r) : r) + 1;
    }
    // The number of t < w with phi(t) < x.
    u64 below(u64 x) const {
        if (x <= lo) return 0;
        const u64 d = x - lo;
        if (!count) return std::min(d, w);
        const u64 i = d / stride, r = d % stride;
        return std::min(i >= count ? count * run : i * run + (sel ? sel->below(r) : std::min(r, run)), w);
    }
    // The walk of the next `limit` chunks that hold a byte of the request (frame.hpp).
    WalkArg walk_arg(const WalkPos & pos, const u8 * in, size_t in_size, u32 limit, u32 rec_base) const {
        return pos.range_arg(in, in_size, lo, hi, limit, rec_base, sel ? 0 : run, stride, count, d_tab, sel ? (u32)sel->m : 0);
    }
    // The gather segment of the decoded chunk in `slot` that holds the frame's bytes [p, p + orig): its wanted bytes are the output bytes
    // [ta, tb) = [below(p), below(p + orig)), contiguous in `out` (and in the base, or nullptr) and one segment, whatever the number of runs or
    // pieces in the chunk; in the chunk they are the bytes c(u) of planes.hpp.  Returns tb, what the frame has committed with this chunk.
    u64 gather(GatherList & g, u64 slot, u64 p, u64 orig, u64 k, u8 * out, const u8 * base) const {
        const u64 ta = below(p), tb = below(p + orig), dst = (u64)(out + ta), b = base ? (u64)(base + ta) : 0;
        if (sel) g.select(slot, orig, k, lo - p, stride, *sel, d_tab, ta / run, ta % run, tb - ta, dst, b);
        else if (count) g.strided(slot, orig, k, lo + (ta / run) * stride + ta % run - p, run - ta % run, run, stride, tb - ta, dst, b);
        else g.range(slot, orig, k, lo + ta - p, lo + tb - p, dst, b);
        return tb;
    }
};

// ---- decompress: n frames whose buffers passed the pointer checks, on device dev ------------------------------------------
// One walk reads every frame header.  Then per window: the walk of the next chunks of the frames in order, up to the
// window's size in all (one launch, one read-back), scatter, run_decode (one CM launch), gather.  Every frame keeps its
// own resume point, committed size and error: a chunk that fails ends its frame alone, the chunks of the frame before it
// are committed; a header error found by the walk ends the frame once the chunks before it are committed.
// bases (or nullptr): per frame nullptr, or base_sizes[i] bytes that are added to the decoded bytes at the same offsets; such a frame's capacity
// is the smaller of out_sizes[i] and base_sizes[i], so that the walk refuses a chunk that runs past the base as one that runs past `out`.
// outs[i] may be bases[i] (planes.hpp, "In place").
// reqs (or nullptr: whole frames, capacity-checked; bz3_hip_decompress_device_{range,strided,select}[_many]): frame i wants the bytes of reqs[i],
// cut at min(out_sizes[i], base_sizes[i]), and nothing is too big.  Its walks are range walks (frame.hpp): chunks that end before the request's
// first byte, or that lie in a gap between two runs or pieces, are header-checked and skipped on the device, headers at or beyond its end() are
// never read, so the windows hold only the chunks that share a byte with their frame's request.  A request in range form walks without a period
// and is gathered clipped at its two ends, one with a period or a piece table walks with it; the tables of a call are uploaded once, beside the
// walk's arguments.  Every chunk is one gather segment (Request::gather) and `committed` counts the request's bytes.  A frame's walk is over at
// its last chunk, at a header error or at the end of its request.
void decompress_frames(int dev, s32 n, const u32 * elem_sizes, const u8 * const * ins, const size_t * in_sizes, const u8 * const * bases, const size_t * base_sizes,
                       u8 * const * outs, size_t * out_sizes, int * rcs, const Request * reqs = nullptr) {
    struct Frame : Request {
        size_t buf_max = 0, committed = 0;  // the capacity (a request: its w)
        u32 decoded = 0;        // chunks decoded and committed
        u32 walked = 0;         // chunks the walks recorded, less those given back (whole frames: pos.done)
        int pending = BZ3_OK;   // the header error the walk stopped at
        bool failed = false;    // a chunk of the current window failed
    };
    struct Chunk {
        s32 frame;
        WalkChunk rec;
    };
    const bool range = reqs != nullptr;
    std::vector<Frame> fr((size_t)n);
    std::vector<WalkPos> pos((size_t)n);
    std::vector<char> live((size_t)n, 0);
    bool any = false;
    std::vector<u64> tables;  // the piece tables of the frames that walk with one, as they are uploaded
    for (s32 i = 0; i < n; i++) {
        rcs[i] = BZ3_OK;
        if (in_sizes[i] < 13) rcs[i] = BZ3_ERR_MALFORMED_HEADER;  // :930
        else live[i] = any = 1;
        fr[i].buf_max = bases && bases[i] ? std::min(out_sizes[i], base_sizes[i]) : out_sizes[i];
        if (range) {
            static_cast<Request &>(fr[i]) = reqs[i];
            fr[i].cut(fr[i].buf_max);
            fr[i].buf_max = (size_t)fr[i].w;
            if (fr[i].sel) {
                fr[i].d_tab = tables.size() * sizeof(u64);
                tables.insert(tables.end(), fr[i].sel->tab.begin(), fr[i].sel->tab.end());
            }
            out_sizes[i] = 0;
        }
    }
    if (!any) return;
    DeviceFrames f;
    std::vector<Chunk> win;
    WalkRound round;
    auto & args = round.args;
    auto & who = round.who;
    auto & rec = round.rec;
    auto & tails = round.tails;
    s32 cur = 0;  // frames before it are finished
    // The next chunks of the live frames from `cur` on, W at most in all, into `win` (frame order).  A frame's limit is what
    // is left of it or of the window; only a frame that stops at a header error walks fewer, and then the frames behind
    // it are walked again with what is left of the window.
    auto collect = [&](size_t W) {
        win.clear();
        while (win.size() < W) {
            if (!round.plain(f, pos, ins, in_sizes, cur, n, (u32)(W - win.size()), [&](s32 i) { return live[i] && fr[i].pending == BZ3_OK; }, [&](s32 i) { return fr[i].buf_max; })) return;
            bool stopped = false;
            for (size_t q = 0; q < who.size(); q++) {
                const s32 i = who[q];
                for (u32 r = 0; r < tails[q].count; r++) win.push_back({i, rec[args[q].rec_base + r]});
                pos[i].take(tails[q]);
                fr[i].walked += tails[q].count;
                if (tails[q].err != BZ3_OK) {
                    fr[i].pending = tails[q].err;
                    stopped = true;
                }
            }
            if (!stopped) return;  // every frame walked its limit: the window is full or no chunk is left
        }
    };
    // The same for ranges.  How many chunks a range touches is known only once they are walked, so every frame gets a limit of what its
    // range would take of full blocks (two more for the two ends), the window's size at most, as long as the walk's records last: 256
    // frames that want one chunk each are one walk and one window.  What a walk finds beyond W goes back to its frames (give_back).
    auto range_walk_over = [&](s32 i) { return pos[i].done == pos[i].n_blocks || pos[i].planned >= fr[i].hi; };
    auto collect_range = [&](size_t W) {
        win.clear();
        while (win.size() < W) {
            args.clear();
            who.clear();
            u32 base = 0;
            for (s32 i = cur; i < n && base < WALK_RECORDS; i++) {
                if (!live[i] || fr[i].pending != BZ3_OK || range_walk_over(i)) continue;
                const u64 from = std::max(fr[i].lo, pos[i].planned), est = (fr[i].hi - from) / pos[i].block_size + 2;
                const u32 lim = (u32)std::min<u64>({est, (u64)(pos[i].n_blocks - pos[i].done), (u64)(W - win.size()), (u64)(WALK_RECORDS - base)});
                args.push_back(fr[i].walk_arg(pos[i], ins[i], in_sizes[i], lim, base));
                who.push_back(i);
                base += lim;
            }
            if (args.empty()) return;
            f.walk(args, rec, tails);
            for (size_t q = 0; q < who.size(); q++) {  // (every frame walked its limit or its walk is over: the loop ends)
                const s32 i = who[q];
                for (u32 r = 0; r < tails[q].count; r++) win.push_back({i, rec[args[q].rec_base + r]});
                pos[i].take(tails[q]);
                fr[i].walked += tails[q].count;
                if (tails[q].err != BZ3_OK) fr[i].pending = tails[q].err;
            }
        }
    };
    // Chunks of `win` beyond the first W go back to their frames (the first window is walked before the states exist).
    auto give_back = [&](size_t W) {
        while (win.size() > W) {
            const Chunk & c = win.back();
            WalkPos & p = pos[c.frame];
            p.off = c.rec.in_off;
            p.planned = c.rec.out_off;
            p.done = c.rec.index;
            fr[c.frame].walked--;
            fr[c.frame].pending = BZ3_OK;  // found again by a later walk
            win.pop_back();
        }
    };
    u32 bs_max = 0;
    try {
        if (!f.open(dev, (size_t)n, tables.size() * sizeof(u64))) throw std::runtime_error("no device");
        DeviceGuard g(dev);
        const u64 d_pieces = f.upload_pieces(tables);
        for (s32 i = 0; i < n; i++)
            if (fr[i].sel) fr[i].d_tab += d_pieces;
        walk_frame_headers(f, n, ins, in_sizes, pos, live, rcs);  // :930-960
        for (s32 i = 0; i < n; i++) {
            if (range && fr[i].buf_max == 0) live[i] = 0;  // nothing wanted: the frame header alone was checked
            if (live[i]) bs_max = std::max(bs_max, pos[i].block_size);
        }
        if (!bs_max) return;
        // n_blocks is untrusted: the states are sized from the chunks the first walk finds present, never from n_blocks
        if (range) collect_range(frame_window_limit());
        else collect(frame_window_limit());
        if (!f.init(bs_max, win.empty() ? 1 : win.size())) throw std::runtime_error("no states");
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (live[i]) rcs[i] = BZ3_ERR_INIT;
        return;
    }
    for (s32 i = 0; i < n; i++)
        if (live[i]) out_sizes[i] = 0;
    try {
        DeviceGuard g(dev);
        const u32 W = (u32)f.states.size();
        std::vector<s32> sizes(W), orig(W);
        std::vector<size_t> caps(W);
        std::vector<void *> slots(W);
        std::vector<u8> hdrs(17 * (size_t)W);
        give_back(W);
        for (bool first = true;; first = false) {
            if (!first && range) collect_range(W), give_back(W);
            else if (!first) collect(W);
            const u32 t = (u32)win.size();
            for (u32 k = 0; k < t; k++) {  // scatter: chunk k to slot k
                const Chunk & c = win[k];
                sizes[k] = c.rec.size;
                orig[k] = c.rec.orig;
                slots[k] = f.slot(k);
                caps[k] = bz3_bound(pos[c.frame].block_size);
                f.states[k]->block_size = (s32)pos[c.frame].block_size;  // every check of the block is made against its own frame's block size
                f.states[k]->last_error = BZ3_OK;
                memcpy(hdrs.data() + 17 * (size_t)k, c.rec.hdr, 17);
                f.gather.plain({(u64)(ins[c.frame] + c.rec.in_off + 8), (u64)f.slot(k), (u64)c.rec.size});
            }
            if (t) {
                f.copy();
                run_decode(f.states.data(), slots.data(), caps.data(), sizes.data(), orig.data(), hdrs.data(), (s32)t, false);
                for (u32 k = 0; k < t; k++) {  // gather: per frame, the chunks before its first failure
                    const Chunk & c = win[k];
                    Frame & x = fr[c.frame];
                    if (x.failed) continue;
                    if (bz3_last_error(f.states[k]) != BZ3_OK) {  // :989-993
                        rcs[c.frame] = f.states[k]->last_error;
                        x.failed = true;
                        continue;
                    }
                    const u64 es = elem_sizes ? (u64)elem_sizes[c.frame] : 1;
                    const u8 * base = bases ? bases[c.frame] : nullptr;
                    if (range) {
                        x.committed = (size_t)x.gather(f.gather, (u64)f.slot(k), c.rec.out_off, (u64)c.rec.orig, es, outs[c.frame], base);
                    } else {
                        f.gather.plain({(u64)f.slot(k), (u64)(outs[c.frame] + c.rec.out_off), (u64)c.rec.orig, es | PLANES_INVERSE, base ? (u64)(base + c.rec.out_off) : 0});
                        x.committed = c.rec.out_off + (size_t)c.rec.orig;
                    }
                    x.decoded++;
                }
                f.copy();
            }
            // a frame ends at a failed chunk, or once every chunk it walked is committed and the walk is over (all chunks, or a header error)
            bool left = false;
            for (s32 i = cur; i < n; i++) {
                if (!live[i]) continue;
                Frame & x = fr[i];
                out_sizes[i] = x.committed;
                if (x.failed) live[i] = 0;
                else if (x.decoded == x.walked && (x.pending != BZ3_OK || pos[i].done == pos[i].n_blocks || (range && range_walk_over(i)))) {
                    rcs[i] = x.pending;
                    live[i] = 0;
                } else {
                    left = true;
                }
            }
            while (cur < n && !live[cur]) cur++;
            if (!left) break;
        }
    } catch (const HipError & e) {
        fprintf(stderr, "bzip3_amd: HIP failure '%s' at %s:%d\n", e.what, e.file, e.line);
        for (s32 i = 0; i < n; i++)
            if (live[i]) rcs[i] = BZ3_ERR_BWT;
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (live[i]) rcs[i] = BZ3_ERR_BWT;
    }
}

// ---- decoded sizes: n frames' chunk headers, walked in rounds of up to WALK_RECORDS chunks over all frames -------------------
void decoded_sizes_frames(int dev, s32 n, const u8 * const * ins, const size_t * in_sizes, size_t * decoded, int * rcs) {
    std::vector<WalkPos> pos((size_t)n);
    std::vector<char> live((size_t)n, 0);
    bool any = false;
    for (s32 i = 0; i < n; i++) {
        decoded[i] = 0;
        rcs[i] = BZ3_OK;
        if (in_sizes[i] < 13) rcs[i] = BZ3_ERR_MALFORMED_HEADER;
        else live[i] = any = 1;
    }
    if (!any) return;
    try {
        DeviceFrames f;
        if (!f.open(dev, (size_t)n)) throw std::runtime_error("no device");
        DeviceGuard g(dev);
        walk_frame_headers(f, n, ins, in_sizes, pos, live, rcs);  // a block size bz3_new refuses: BZ3_ERR_INIT, what bz3_decompress reports for it
        WalkRound round;
        auto unfinished = [&](s32 i) {  // (a frame whose walk is over is done with: no later failure touches its code)
            if (pos[i].done == pos[i].n_blocks) live[i] = 0;
            return live[i] != 0;
        };
        while (round.plain(f, pos, ins, in_sizes, 0, n, (u32)WALK_RECORDS, unfinished, [](s32) { return (size_t)SIZE_MAX; })) {
            for (size_t q = 0; q < round.who.size(); q++) {
                const s32 i = round.who[q];
                pos[i].take(round.tails[q]);
                decoded[i] = pos[i].planned;
                if (round.tails[q].err != BZ3_OK) {
                    rcs[i] = round.tails[q].err;
                    live[i] = 0;
                }
            }
        }
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (live[i]) rcs[i] = BZ3_ERR_INIT;
    }
}

// ---- update: n frames whose buffers passed the pointer checks, on device dev ------------------------------------------------------
// Frame i's decoded bytes [offsets[i], offsets[i] + ws[i]) get the values datas[i][0, ws[i]) (less bases[i][0, ws[i]) where there is a base) and
// the new frame goes to outs[i] (bz3_hip.h, "Range update").  Only the chunks that share a byte with the range (the touched ones) are coded again;
// of those only the ones the range cuts are decoded first, the others are rebuilt from the new bytes alone; everything else of the frame is copied.
//   1. One walk reads every frame header, then plain walks read every chunk header of every frame (rounds of WALK_RECORDS chunks over all
//      frames).  They give T, the frame's end, `need`, and the records of the touched chunks, which are all that is kept.
//   2. The touched chunks of all frames form one list in frame order and go through windows of as many slots as the call has states (sized from
//      the list, never from n_blocks).  Before anything is written to an `out`, every cut chunk of the call is decoded whole.  Where the list
//      fits one window (the usual row update) those decodes already sit in their chunks' slots; a longer list decodes its cut chunks once to
//      check them, a window at a time, and again in the window that codes them (at most two chunks per frame).
//   3. Per window: (the cut chunks' coded bytes into their slots, run_decode on that subset: the slot then holds the chunk in split form;) ONE
//      patch launch -- a whole-block split from `data` for a covered chunk, a clipped split for a cut one --; run_encode on the window's slots;
//      one pack launch: the new chunk headers from the staged buffer, the coded slots, and the verbatim runs.  The bytes of a frame before its
//      first touched chunk (the frame header among them) are contiguous in `in` and in `out`, and so are those behind its last one: two plain
//      segments per frame.  (A frame may hold empty chunks between touched ones; each such gap is a run of its own, and the launch is split
//      where its table is full.)
// A frame that fails in 1 or 2 has its code, size 0 and an untouched `out`; one that fails in 3 (not expected) its code and size 0.
// The bytes to replace are those of reqs[i], cut at ws[i] (bz3_hip.h, "Index update"): a request in range form is the range above, bit for bit; one
// with a piece table names the bytes phi(t), t < w, and data[t] (base[t]) pairs with phi(t).  Whatever the form, chunk j's new bytes are
// data[ta, tb) with ta = below(p_j), tb = below(p_j + o_j): one contiguous piece of data and of base.  It is touched iff tb > ta, covered iff
// tb - ta == o_j and cut otherwise, and a cut chunk is decoded once however many pieces and periods it holds.  Its patch segment is a whole split,
// a clipped split where its new bytes are one run of the chunk, and a select split otherwise (GatherList::patch_select); the piece tables of a call
// are uploaded once, beside the walk's arguments, as decompress_frames uploads them.  The walk stays the plain walk: the copies need every record.
// A call whose touched chunks exceed one window still decodes its cut chunks twice; parking the decoded chunks is open.
// Sync (olds != nullptr; bz3_hip.h, "Sync"): every request is the range (0, ws[i]), datas[i] is the whole new tensor and olds[i] what the frame
// decodes to.  The touched chunks are then the DIRTY ones: every walk round's records become one diff table (a segment per chunk with a byte,
// data[p_j, p_j + o_j) against old[p_j, p_j + o_j); a chunk that runs past ws[i] is left out, its frame fails with T != ws[i] below), one
// k_diff_segments launch and one read-back of the round's flags, before the round's records are looked at.  A dirty chunk has ta = p_j and
// tb = p_j + o_j, so it is covered: no chunk of a sync is cut, the decode lambda below is never reached, and everything from 2 on is the update's
// own path.  recoded[i] (recoded may be nullptr) is the frame's number of dirty chunks, 0 for a frame that fails before a write.
void update_frames(int dev, s32 n, const u32 * elem_sizes, const u8 * const * ins, const size_t * in_sizes, const Request * reqs, const u8 * const * datas,
                   const size_t * ws, const u8 * const * bases, u8 * const * outs, size_t * out_sizes, int * rcs, const u8 * const * olds = nullptr,
                   u32 * recoded = nullptr) {
    struct Frame : Request {    // cut at ws[i]: w bytes, the last of them phi(w - 1) = hi - 1 (hi == UINT64_MAX: it does not fit 64 bits)
        u64 need = 13, tail = 0;  // the capacity the frame needs; the offset behind its last chunk
        size_t cap = 0, pos = 0;
        u64 in_next = 0;         // the frame's bytes before it are in `out`
        u32 chunks = 0, packed = 0;  // its touched chunks, and those of them that are packed
    };
    struct Touched {
        s32 frame;
        WalkChunk rec;
        u64 ta, tb;  // the chunk's new bytes are data[ta, tb) (Request::below of its two ends), of base too
        bool cut() const { return tb - ta != (u64)rec.orig; }
    };
    std::vector<u64> tables;  // the piece tables of the frames that patch with one, as they are uploaded
    std::vector<Frame> fr((size_t)n);
    std::vector<WalkPos> pos((size_t)n);
    std::vector<char> live((size_t)n, 0);
    std::vector<Touched> touch;
    bool any = false;
    for (s32 i = 0; i < n; i++) {
        rcs[i] = BZ3_OK;
        if (recoded) recoded[i] = 0;
        fr[i].cap = out_sizes[i];
        out_sizes[i] = 0;
        static_cast<Request &>(fr[i]) = reqs[i];
        fr[i].cut((u64)ws[i]);
        if (fr[i].sel) {
            fr[i].d_tab = tables.size() * sizeof(u64);
            tables.insert(tables.end(), fr[i].sel->tab.begin(), fr[i].sel->tab.end());
        }
        if (in_sizes[i] < 13) rcs[i] = BZ3_ERR_MALFORMED_HEADER;  // :930
        else live[i] = any = 1;
    }
    if (!any) return;
    auto fail = [&](s32 i, int rc) {
        rcs[i] = rc;
        out_sizes[i] = 0;
        live[i] = 0;
    };
    DeviceFrames f;
    u32 bs_max = 0;
    try {
        if (!f.open(dev, (size_t)n, tables.size() * sizeof(u64), 2, olds ? WALK_RECORDS : 0)) throw std::runtime_error("no device");
        DeviceGuard g(dev);
        const u64 d_pieces = f.upload_pieces(tables);
        for (s32 i = 0; i < n; i++)
            if (fr[i].sel) fr[i].d_tab += d_pieces;
        walk_frame_headers(f, n, ins, in_sizes, pos, live, rcs);  // :930-960
        WalkRound round;
        std::vector<CopySeg> diffs;  // a sync's diff table of the round, and its flags, one per record
        std::vector<u32> dirty;
        // every chunk header of every live frame
        while (round.plain(f, pos, ins, in_sizes, 0, n, (u32)WALK_RECORDS, [&](s32 i) { return live[i] != 0; }, [](s32) { return (size_t)SIZE_MAX; })) {
            if (olds) {
                diffs.clear();
                dirty.resize(round.rec.size());
                for (size_t q = 0; q < round.who.size(); q++) {
                    const s32 i = round.who[q];
                    for (u32 r = 0; r < round.tails[q].count && datas[i] != olds[i]; r++) {
                        const WalkChunk & c = round.rec[round.args[q].rec_base + r];
                        const u64 p = c.out_off, o = (u64)c.orig;
                        if (o > 0 && p + o <= fr[i].w) diffs.push_back({(u64)(datas[i] + p), 0, o, (u64)(round.args[q].rec_base + r), (u64)(olds[i] + p)});
                    }
                }
                diff_segments(diffs, f.staging, f.meta + f.lay.diff, (u32 *)(f.meta + f.lay.flags), dirty.data(), dirty.size(), f.s);
            }
            for (size_t q = 0; q < round.who.size(); q++) {
                const s32 i = round.who[q];
                const WalkTail & tail = round.tails[q];
                Frame & x = fr[i];
                for (u32 r = 0; r < tail.count; r++) {
                    const WalkChunk & c = round.rec[round.args[q].rec_base + r];
                    const u64 p = c.out_off, o = (u64)c.orig;
                    const u64 ta = o > 0 ? x.below(p) : 0, tb = o > 0 ? x.below(p + o) : 0;  // (touched iff the chunk holds phi(t) for some t < w)
                    const bool touched = olds ? dirty[round.args[q].rec_base + r] != 0 : tb > ta;
                    x.need += 8 + (touched ? (u64)bz3_bound((size_t)o) : (u64)c.size);
                    if (!touched) continue;
                    touch.push_back({i, c, ta, tb});
                    x.chunks++;
                }
                pos[i].take(tail);
                if (tail.err != BZ3_OK) fail(i, tail.err);
            }
        }
        for (s32 i = 0; i < n; i++) {
            if (!live[i]) continue;
            fr[i].tail = pos[i].off;
            if (fr[i].hi > pos[i].planned || (olds && fr[i].w != pos[i].planned) || fr[i].cap < fr[i].need) fail(i, BZ3_ERR_DATA_TOO_BIG);
            else if (recoded) recoded[i] = fr[i].chunks;
        }
        touch.erase(std::remove_if(touch.begin(), touch.end(), [&](const Touched & t) { return !live[t.frame]; }), touch.end());
        for (const Touched & t : touch) bs_max = std::max(bs_max, pos[t.frame].block_size);
        if (bs_max && !f.init(bs_max, std::min(touch.size(), FRAME_WINDOW_MAX))) throw std::runtime_error("no states");
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (live[i]) fail(i, BZ3_ERR_INIT);
        return;
    }
    try {
        DeviceGuard g(dev);
        const size_t total = touch.size(), W = std::max<size_t>(f.states.size(), 1);
        const bool one_window = total <= W;
        std::vector<bz3_state *> sts;
        std::vector<void *> slots;
        std::vector<s32> sizes, orig, which;
        std::vector<size_t> caps;
        std::vector<u8> hdrs, hdr;
        // Decodes the chunks jobs[j] = (index into touch, slot) in place in their slots: one copy launch and one run_decode.  A chunk that fails
        // ends its frame.
        auto decode = [&](const std::vector<std::pair<size_t, size_t>> & jobs) {
            if (jobs.empty()) return;
            sts.clear(), slots.clear(), sizes.clear(), orig.clear(), caps.clear(), hdrs.clear();
            for (const auto & [t, k] : jobs) {
                const Touched & c = touch[t];
                f.states[k]->block_size = (s32)pos[c.frame].block_size;  // every check of the block is made against its own frame's block size
                f.states[k]->last_error = BZ3_OK;
                sts.push_back(f.states[k]);
                slots.push_back(f.slot(k));
                sizes.push_back(c.rec.size);
                orig.push_back(c.rec.orig);
                caps.push_back(bz3_bound(pos[c.frame].block_size));
                hdrs.insert(hdrs.end(), c.rec.hdr, c.rec.hdr + 17);
                f.gather.plain({(u64)(ins[c.frame] + c.rec.in_off + 8), (u64)f.slot(k), (u64)c.rec.size});
                if (f.gather.size() == f.lay.segs) f.copy();
            }
            f.copy();
            run_decode(sts.data(), slots.data(), caps.data(), sizes.data(), orig.data(), hdrs.data(), (s32)jobs.size(), false);
            for (size_t j = 0; j < jobs.size(); j++)
                if (live[touch[jobs[j].first].frame] && bz3_last_error(sts[j]) != BZ3_OK) fail(touch[jobs[j].first].frame, sts[j]->last_error);
        };
        std::vector<std::pair<size_t, size_t>> jobs;
        for (size_t t = 0; t < total; t++) {  // every cut chunk of the call, before any write to an `out`
            if (touch[t].cut()) jobs.push_back({t, one_window ? t : jobs.size()});
            if (jobs.size() == W || t + 1 == total) {
                decode(jobs);
                jobs.clear();
            }
        }
        auto flush = [&]() {  // the pack launch (a part of it, where its table is full)
            f.stage_headers(hdr);
            f.copy();
            hdr.clear();
        };
        auto run = [&](s32 i, u64 from, u64 to) {  // the frame's bytes [from, to) verbatim, behind what `out` holds
            if (to > from) {
                if (f.gather.size() + 3 > f.lay.segs) flush();
                f.gather.plain({(u64)(ins[i] + from), (u64)(outs[i] + fr[i].pos), to - from});
            }
            fr[i].pos += (size_t)(to - from);
            fr[i].in_next = to;
        };
        for (s32 i = 0; i < n; i++)  // a frame without a touched chunk is one run
            if (live[i] && fr[i].chunks == 0) {
                run(i, 0, fr[i].tail);
                out_sizes[i] = fr[i].pos;
            }
        for (size_t w0 = 0; w0 < total; w0 += W) {
            const size_t cnt = std::min(W, total - w0);
            if (!one_window) {
                jobs.clear();
                for (size_t k = 0; k < cnt; k++)
                    if (touch[w0 + k].cut() && live[touch[w0 + k].frame]) jobs.push_back({w0 + k, k});
                if (!f.gather.v.empty()) flush();  // (the runs collected so far: the decode's scatter is a launch of its own)
                decode(jobs);
            }
            // patch: the new bytes into the slots, split
            if (!f.gather.v.empty()) flush();
            sts.clear(), slots.clear(), sizes.clear(), which.clear();
            for (size_t k = 0; k < cnt; k++) {
                const Touched & c = touch[w0 + k];
                const s32 i = c.frame;
                if (!live[i]) continue;
                const Frame & x = fr[i];
                const u64 p = c.rec.out_off, es = elem_sizes ? (u64)elem_sizes[i] : 1;
                const u64 src = (u64)(datas[i] + c.ta), b = bases && bases[i] ? (u64)(bases[i] + c.ta) : 0;  // the chunk's first new byte in data and base
                if (x.sel) f.gather.patch_select(src, b, (u64)f.slot(k), (u64)c.rec.orig, es, x.lo - p, x.stride, *x.sel, x.d_tab, c.ta / x.run, c.ta % x.run, c.tb - c.ta);
                else f.gather.patch(src, b, (u64)f.slot(k), (u64)c.rec.orig, es, x.lo + c.ta - p, x.lo + c.tb - p);
                f.states[k]->block_size = (s32)pos[i].block_size;
                f.states[k]->last_error = BZ3_OK;
                sts.push_back(f.states[k]);
                slots.push_back(f.slot(k));
                sizes.push_back(c.rec.orig);
                which.push_back((s32)k);
            }
            if (sts.empty()) continue;
            f.copy();
            run_encode(sts.data(), slots.data(), sizes.data(), (s32)sts.size(), false);
            // pack
            for (size_t j = 0; j < which.size(); j++) {
                const Touched & c = touch[w0 + (size_t)which[j]];
                const s32 i = c.frame;
                Frame & x = fr[i];
                if (!live[i]) continue;  // an earlier block of its frame failed in this window
                const s32 osz = sizes[j];
                if (bz3_last_error(sts[j]) != BZ3_OK || osz < 0 || (size_t)osz > bz3_bound((size_t)c.rec.orig)) {
                    fail(i, bz3_last_error(sts[j]) != BZ3_OK ? sts[j]->last_error : BZ3_ERR_DATA_TOO_BIG);
                    continue;
                }
                run(i, x.in_next, c.rec.in_off);  // the frame header and the chunks before its first touched one, or the empty chunks in a gap
                if (f.gather.size() + 3 > f.lay.segs || hdr.size() + 8 > f.lay.tab - f.lay.hdr) flush();
                const size_t h = hdr.size();
                hdr.resize(h + 8);
                wr_le32(hdr.data() + h, (u32)osz);
                wr_le32(hdr.data() + h + 4, (u32)c.rec.orig);
                f.gather.plain({(u64)(f.meta + f.lay.hdr + h), (u64)(outs[i] + x.pos), 8});
                f.gather.plain({(u64)slots[j], (u64)(outs[i] + x.pos + 8), (u64)osz});
                x.pos += (size_t)osz + 8;
                x.in_next = c.rec.in_off + 8 + (u64)c.rec.size;
                if (++x.packed == x.chunks) {
                    run(i, x.in_next, x.tail);
                    out_sizes[i] = x.pos;
                }
            }
            flush();
        }
        if (!f.gather.v.empty()) flush();
    } catch (const HipError & e) {
        fprintf(stderr, "bzip3_amd: HIP failure '%s' at %s:%d\n", e.what, e.file, e.line);
        for (s32 i = 0; i < n; i++)
            if (live[i] && (fr[i].packed < fr[i].chunks || !out_sizes[i])) fail(i, BZ3_ERR_BWT);
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (live[i] && (fr[i].packed < fr[i].chunks || !out_sizes[i])) fail(i, BZ3_ERR_BWT);
    }
}

// ---- resize: n frames whose buffers passed the pointer checks, on device dev ------------------------------------------------------
// The effective block size bz3_compress codes t bytes with under `block_size` (src/libbz3.c:877-878), in 64 bits.
u64 effective_block_size(u32 block_size, u64 t) {
    const u64 bs = (u64)block_size > t ? (u64)t + t / 50 + 32 : (u64)block_size;  // (bz3_bound, which may not fit size_t's callers' 32 bits)
    return std::max<u64>(bs, (u64)KiB65);
}

// Frame i keeps the first keeps[i] bytes of what it decodes to, gets datas[i][0, ws[i]) behind them (less bases[i][0, ws[i]) where there is a base)
// and the new frame goes to outs[i] (bz3_hip.h, "Resize").  T' = keep + w and B = eff(block_size, T') are known before the walk; new chunk c is
// [c B, min((c + 1) B, T')).
//   1. One walk reads every frame header, then plain walks read every chunk header of every frame, as the update's do.  They give T, tell a regular
//      frame from any other, and give the copied prefix: with the header's block size equal to B, the old chunks that end at or below keep and
//      have the extent of the new chunk of their number.  Everything behind them is rebuilt.  The first rebuilt chunk holds kept bytes iff it
//      starts below keep; they are the first a = min(keep, its end) - its start bytes of it AND of the one old chunk that starts where it does
//      (the same number under one block size; chunk 0 on both sides where the block size changes, which takes a frame of one chunk on one side).
//      That old chunk is the frame's cut chunk; no other chunk of the frame is decoded.
//   2. The rebuilt chunks of all frames form one list in frame order and go through windows of as many slots as the call has states.  Before
//      anything is written to an `out`, every cut chunk of the call is decoded whole; where the list fits one window those decodes are the ones the
//      window uses, a longer list decodes them once to check them and again in the window that codes them (one chunk per frame).
//   3. Per window: the cut chunks into the parking slots (k = 1: into the chunk's own slot, which needs no move) and run_decode on them; ONE patch
//      launch -- a replane segment from the parking slot for the kept head, a clipped or whole split from `data` for the rest --; run_encode; one
//      pack launch: the new frame header and the new chunk headers from the staged buffer, the coded slots, and per frame one verbatim run, the
//      copied chunks, which are a prefix.
// A frame that fails in 1 or 2 has its code, size 0 and an untouched `out`; one that fails in 3 (not expected) its code and size 0.
void resize_frames(int dev, s32 n, const u32 * block_sizes, const u32 * elem_sizes, const u8 * const * ins, const size_t * in_sizes, const u64 * keeps,
                   const u8 * const * datas, const size_t * ws, const u8 * const * bases, u8 * const * outs, size_t * out_sizes, int * rcs) {
    struct Frame {
        u64 keep = 0, Tn = 0, B = 0;       // T' and the new block size
        u64 need = 13, copy_end = 13;      // the capacity the frame needs; the end of its copied chunks in `in`
        u32 ncopy = 0, chunks = 0, packed = 0;  // copied chunks; rebuilt chunks and those of them that are packed
        u64 nb = 0;                        // new chunks
        bool regular = true, has_cut = false, started = false;
        WalkChunk cut{};                   // the old chunk that holds the kept bytes of the first rebuilt chunk
        size_t cap = 0, pos = 0;
    };
    struct Rebuilt {
        s32 frame;
        u64 start, size, a;  // the new chunk's first byte and size; its kept bytes (those of the frame's cut chunk)
    };
    std::vector<Frame> fr((size_t)n);
    std::vector<WalkPos> pos((size_t)n);
    std::vector<char> live((size_t)n, 0);
    std::vector<Rebuilt> list;
    bool any = false;
    for (s32 i = 0; i < n; i++) {
        rcs[i] = BZ3_OK;
        Frame & x = fr[i];
        x.cap = out_sizes[i];
        out_sizes[i] = 0;
        x.keep = keeps ? keeps[i] : 0;
        x.Tn = x.keep + (u64)ws[i];
        if (x.Tn < x.keep) rcs[i] = BZ3_ERR_DATA_TOO_BIG;  // (keep + w does not fit 64 bits: keep > T whatever T is)
        else if (in_sizes[i] < 13) rcs[i] = BZ3_ERR_MALFORMED_HEADER;  // :930
        else live[i] = any = 1;
        x.B = effective_block_size(block_sizes[i], x.Tn);
        x.nb = (x.Tn + x.B - 1) / x.B;
    }
    if (!any) return;
    auto fail = [&](s32 i, int rc) {
        rcs[i] = rc;
        out_sizes[i] = 0;
        live[i] = 0;
    };
    auto new_size = [&](const Frame & x, u64 c) { return std::min(x.B, x.Tn - c * x.B); };  // of new chunk c < nb
    DeviceFrames f;
    u8 * park = nullptr;  // the slots the cut chunks with k > 1 are decoded into, one per such chunk of a window
    u32 bs_max = 0;
    try {
        if (!f.open(dev, (size_t)n, 0, 2)) throw std::runtime_error("no device");
        DeviceGuard g(dev);
        walk_frame_headers(f, n, ins, in_sizes, pos, live, rcs);  // :930-960
        WalkRound round;
        while (round.plain(f, pos, ins, in_sizes, 0, n, (u32)WALK_RECORDS, [&](s32 i) { return live[i] != 0; }, [](s32) { return (size_t)SIZE_MAX; })) {
            for (size_t q = 0; q < round.who.size(); q++) {
                const s32 i = round.who[q];
                const WalkTail & tail = round.tails[q];
                Frame & x = fr[i];
                const u64 bs = pos[i].block_size;
                for (u32 r = 0; r < tail.count; r++) {
                    const WalkChunk & c = round.rec[round.args[q].rec_base + r];
                    const u64 p = c.out_off, o = (u64)c.orig;
                    const bool last = c.index + 1 == pos[i].n_blocks;
                    if (p != (u64)c.index * bs || o == 0 || o > bs || (!last && o != bs)) x.regular = false;
                    if (!x.regular) continue;
                    if (bs == x.B && c.index == x.ncopy && p + o <= x.keep && (u64)c.index < x.nb && o == new_size(x, c.index)) {
                        x.ncopy++;
                        x.need += 8 + (u64)c.size;
                        x.copy_end = c.in_off + 8 + (u64)c.size;
                    } else if (x.keep > 0 && p <= x.keep - 1 && x.keep - 1 < p + o) {
                        x.cut = c;
                        x.has_cut = true;
                    }
                }
                pos[i].take(tail);
                if (tail.err != BZ3_OK) fail(i, tail.err);
            }
        }
        size_t parked = 0;  // the cut chunks with k > 1 of the call: one per frame at most, and a window holds no more of them than it has slots
        for (s32 i = 0; i < n; i++) {
            if (!live[i]) continue;
            Frame & x = fr[i];
            const u64 T = pos[i].planned;
            if (!x.regular || (u64)pos[i].block_size != effective_block_size(block_sizes[i], T) || (pos[i].n_blocks == 0) != (T == 0)) {
                fail(i, BZ3_ERR_INIT);
                continue;
            }
            if (x.keep > T) {
                fail(i, BZ3_ERR_DATA_TOO_BIG);
                continue;
            }
            if (x.B > (u64)MiB511 || (x.Tn >= x.B && x.Tn % x.B == 0)) {  // bz3_new's limit; the block src/libbz3.c:914 would drop
                fail(i, BZ3_ERR_INIT);
                continue;
            }
            for (u64 c = x.ncopy; c < x.nb; c++) x.need += 8 + (u64)bz3_bound((size_t)new_size(x, c));
            if (x.cap < x.need) {
                fail(i, BZ3_ERR_DATA_TOO_BIG);
                continue;
            }
            for (u64 c = x.ncopy; c < x.nb; c++) {
                const u64 start = c * x.B, size = new_size(x, c), a = start < x.keep ? std::min(x.keep, start + size) - start : 0;
                if (a && (!x.has_cut || x.cut.out_off != start || c != x.ncopy || a > (u64)x.cut.orig)) throw std::logic_error("kept bytes without their chunk");
                if (a && (elem_sizes ? elem_sizes[i] : 1) > 1) parked++;
                list.push_back({i, start, size, a});
                x.chunks++;
                bs_max = std::max(bs_max, (u32)x.B);
                if (a) bs_max = std::max(bs_max, pos[i].block_size);
            }
        }
        if (bs_max && !f.init(bs_max, std::min(list.size(), FRAME_WINDOW_MAX))) throw std::runtime_error("no states");
        if (parked) {
            HIP_CHECK(hipSetDevice(dev));
            HIP_CHECK(hipMalloc((void **)&park, std::min(parked, f.states.size()) * f.stride));
        }
    } catch (...) {
        if (park) (void)hipFree(park);
        for (s32 i = 0; i < n; i++)
            if (live[i]) fail(i, BZ3_ERR_INIT);
        return;
    }
    try {
        DeviceGuard g(dev);
        const size_t total = list.size(), W = std::max<size_t>(f.states.size(), 1);
        const bool one_window = total <= W;
        std::vector<bz3_state *> sts;
        std::vector<void *> slots, where(W, nullptr);  // where[k]: the decoded cut chunk of the window's chunk k
        std::vector<s32> sizes, orig, which;
        std::vector<size_t> caps;
        std::vector<u8> hdrs, hdr;
        // Decodes the cut chunks of the frames of jobs[j] = (index into list, state, destination): one copy launch and one run_decode.  A chunk that
        // fails ends its frame.
        struct Job {
            size_t t, k;
            u8 * to;
        };
        auto decode = [&](const std::vector<Job> & jobs) {
            if (jobs.empty()) return;
            sts.clear(), slots.clear(), sizes.clear(), orig.clear(), caps.clear(), hdrs.clear();
            for (const Job & j : jobs) {
                const s32 i = list[j.t].frame;
                const WalkChunk & c = fr[i].cut;
                f.states[j.k]->block_size = (s32)pos[i].block_size;  // every check of the block is made against its own frame's block size
                f.states[j.k]->last_error = BZ3_OK;
                sts.push_back(f.states[j.k]);
                slots.push_back(j.to);
                sizes.push_back(c.size);
                orig.push_back(c.orig);
                caps.push_back(bz3_bound(pos[i].block_size));
                hdrs.insert(hdrs.end(), c.hdr, c.hdr + 17);
                f.gather.plain({(u64)(ins[i] + c.in_off + 8), (u64)j.to, (u64)c.size});
                if (f.gather.size() == f.lay.segs) f.copy();
            }
            f.copy();
            run_decode(sts.data(), slots.data(), caps.data(), sizes.data(), orig.data(), hdrs.data(), (s32)jobs.size(), false);
            for (size_t j = 0; j < jobs.size(); j++)
                if (live[list[jobs[j].t].frame] && bz3_last_error(sts[j]) != BZ3_OK) fail(list[jobs[j].t].frame, sts[j]->last_error);
        };
        // The jobs of the window [w0, w0 + cnt): a chunk with k > 1 is decoded into the next parking slot, one with k = 1 into its own slot.
        std::vector<Job> jobs;
        auto window_jobs = [&](size_t w0, size_t cnt) {
            jobs.clear();
            size_t p = 0;
            for (size_t k = 0; k < cnt; k++) {
                const Rebuilt & c = list[w0 + k];
                where[k] = nullptr;
                if (!c.a || !live[c.frame]) continue;
                where[k] = (elem_sizes ? elem_sizes[c.frame] : 1) > 1 ? park + (p++) * f.stride : f.slot(k);
                jobs.push_back({w0 + k, k, (u8 *)where[k]});
            }
        };
        if (one_window) {
            window_jobs(0, total);
            decode(jobs);
        } else {  // every cut chunk of the call, before any write to an `out`: into the slots, to be checked alone
            jobs.clear();
            for (size_t t = 0; t < total; t++) {
                if (list[t].a) jobs.push_back({t, jobs.size(), f.slot(jobs.size())});
                if (jobs.size() == W || t + 1 == total) {
                    decode(jobs);
                    jobs.clear();
                }
            }
        }
        auto flush = [&]() {  // the pack launch (a part of it, where its table is full)
            f.stage_headers(hdr);
            f.copy();
            hdr.clear();
        };
        // The frame's 13 header bytes and its copied chunks, once, before its first rebuilt chunk (or alone).
        auto start = [&](s32 i) {
            Frame & x = fr[i];
            if (x.started) return;
            if (f.gather.size() + 4 > f.lay.segs || hdr.size() + 21 > f.lay.tab - f.lay.hdr) flush();
            const size_t h = hdr.size();
            hdr.insert(hdr.end(), {'B', 'Z', '3', 'v', '1'});
            hdr.resize(h + 13);
            wr_le32(hdr.data() + h + 5, (u32)x.B);
            wr_le32(hdr.data() + h + 9, (u32)x.nb);
            f.gather.plain({(u64)(f.meta + f.lay.hdr + h), (u64)outs[i], 13});
            if (x.copy_end > 13) f.gather.plain({(u64)(ins[i] + 13), (u64)(outs[i] + 13), x.copy_end - 13});
            x.pos = (size_t)x.copy_end;
            x.started = true;
        };
        for (s32 i = 0; i < n; i++)  // a frame without a rebuilt chunk is its header and one run
            if (live[i] && fr[i].chunks == 0) {
                start(i);
                out_sizes[i] = fr[i].pos;
            }
        for (size_t w0 = 0; w0 < total; w0 += W) {
            const size_t cnt = std::min(W, total - w0);
            if (!f.gather.v.empty()) flush();  // (the runs collected so far: the launches below are of other kinds)
            if (!one_window) {
                window_jobs(w0, cnt);
                decode(jobs);
            }
            // patch: the kept head from where it was decoded, the new bytes from `data`, split
            sts.clear(), slots.clear(), sizes.clear(), which.clear();
            for (size_t k = 0; k < cnt; k++) {
                const Rebuilt & c = list[w0 + k];
                const s32 i = c.frame;
                if (!live[i]) continue;
                const Frame & x = fr[i];
                const u64 es = elem_sizes ? (u64)elem_sizes[i] : 1, from = c.start + c.a - x.keep;  // the chunk's first new byte in data and base
                if (c.a) f.gather.replane((u64)where[k], (u64)f.slot(k), (u64)x.cut.orig, c.size, es, c.a);
                f.gather.patch((u64)(datas[i] + from), bases && bases[i] ? (u64)(bases[i] + from) : 0, (u64)f.slot(k), c.size, es, c.a, c.size);
                f.states[k]->block_size = (s32)x.B;
                f.states[k]->last_error = BZ3_OK;
                sts.push_back(f.states[k]);
                slots.push_back(f.slot(k));
                sizes.push_back((s32)c.size);
                which.push_back((s32)k);
            }
            if (sts.empty()) continue;
            f.copy();
            run_encode(sts.data(), slots.data(), sizes.data(), (s32)sts.size(), false);
            // pack
            for (size_t j = 0; j < which.size(); j++) {
                const Rebuilt & c = list[w0 + (size_t)which[j]];
                const s32 i = c.frame;
                Frame & x = fr[i];
                if (!live[i]) continue;  // an earlier block of its frame failed in this window
                const s32 osz = sizes[j];
                if (bz3_last_error(sts[j]) != BZ3_OK || osz < 0 || (size_t)osz > bz3_bound((size_t)c.size)) {
                    fail(i, bz3_last_error(sts[j]) != BZ3_OK ? sts[j]->last_error : BZ3_ERR_DATA_TOO_BIG);
                    continue;
                }
                start(i);
                if (f.gather.size() + 2 > f.lay.segs || hdr.size() + 8 > f.lay.tab - f.lay.hdr) flush();
                const size_t h = hdr.size();
                hdr.resize(h + 8);
                wr_le32(hdr.data() + h, (u32)osz);
                wr_le32(hdr.data() + h + 4, (u32)c.size);
                f.gather.plain({(u64)(f.meta + f.lay.hdr + h), (u64)(outs[i] + x.pos), 8});
                f.gather.plain({(u64)slots[j], (u64)(outs[i] + x.pos + 8), (u64)osz});
                x.pos += (size_t)osz + 8;
                if (++x.packed == x.chunks) out_sizes[i] = x.pos;
            }
            flush();
        }
        if (!f.gather.v.empty()) flush();
    } catch (const HipError & e) {
        fprintf(stderr, "bzip3_amd: HIP failure '%s' at %s:%d\n", e.what, e.file, e.line);
        for (s32 i = 0; i < n; i++)
            if (live[i] && (fr[i].packed < fr[i].chunks || !out_sizes[i])) fail(i, BZ3_ERR_BWT);
    } catch (...) {
        for (s32 i = 0; i < n; i++)
            if (live[i] && (fr[i].packed < fr[i].chunks || !out_sizes[i])) fail(i, BZ3_ERR_BWT);
    }
    if (park) {
        (void)hipStreamSynchronize(f.s);
        (void)hipFree(park);
    }
}

// ---- the entry points' argument checks ------------------------------------------------------------------------------------
// The GPU of a call: every non-empty buffer (a[i] with a_sizes[i] > 0, likewise b) must be device memory of the GPU the first
// one lives on.  -1: no buffer is non-empty; -2: one is not.
int frames_device(s32 n, const void * const * a, const size_t * a_sizes, const void * const * b, const size_t * b_sizes) {
    int dev = -1;
    auto check = [&](const void * p) {
        const int d = device_of(p);
        if (d < 0 || (dev >= 0 && d != dev)) return false;
        dev = d;
        return true;
    };
    for (s32 i = 0; i < n; i++) {
        if (a_sizes[i] && !check(a[i])) return -2;
        if (b && b_sizes[i] && !check(b[i])) return -2;
    }
    return dev;
}

// Whole-call failure: every frame gets `rc` and size 0.
int fail_frames(s32 n, int * rcs, size_t * sizes, int rc) {
    for (s32 i = 0; i < n; i++) {
        if (rcs) rcs[i] = rc;
        if (sizes) sizes[i] = 0;
    }
    return rc;
}

int first_error(s32 n, const int * rcs) {
    for (s32 i = 0; i < n; i++)
        if (rcs[i] != BZ3_OK) return rcs[i];
    return BZ3_OK;
}

// Do [a, a + a_size) and [b, b + b_size) share a byte?
bool ranges_overlap(const void * a, size_t a_size, const void * b, size_t b_size) {
    const u64 x = (u64)a, y = (u64)b;
    return a_size && b_size && x < y + b_size && y < x + a_size;
}

bool elem_sizes_ok(s32 n, const u32 * elem_sizes) {
    for (s32 i = 0; i < n; i++)
        if (!planes_elem_size_ok(elem_sizes[i])) return false;
    return true;
}


// The front of the partial decode and the update calls over n > 0 frames: the whole-call checks they share (args_ok: the caller's own pointers and
// parameters), frame i's request from make(i, request) (false: an invalid one), and in `dev` the call's device as frames_device names it, which the
// caller judges by its own rule.  False: the call fails, before any write, with BZ3_ERR_INIT.
bool request_front(s32 n, const u32 * elem_sizes, const void * const * ins, const size_t * in_sizes, bool args_ok, void * const * outs, size_t * out_sizes, int * rcs,
                   const std::function<bool(s32, Request &)> & make, std::vector<Request> & reqs, int & dev) {
    if (n < 0 || !ins || !in_sizes || !outs || !out_sizes || !rcs || !args_ok) return false;
    if (elem_sizes && !elem_sizes_ok(n, elem_sizes)) return false;
    reqs.resize((size_t)n);
    for (s32 i = 0; i < n; i++)
        if (!make(i, reqs[(size_t)i])) return false;
    dev = frames_device(n, ins, in_sizes, (const void * const *)outs, out_sizes);
    return true;
}

// Frame i's index set of a select call, params[4 i ..] = (offset, stride, count, m) and the m pairs (s_j, l_j) of pieces[i] in host memory, into t.
// False for a set that bz3_hip.h calls invalid; else W = count L, the bytes it names (0: none, and offset and stride were not looked at).
bool read_index_set(const u64 * params, const u64 * const * pieces, s32 i, PieceTable & t, u64 & W) {
    const u64 offset = params[4 * i], stride = params[4 * i + 1], count = params[4 * i + 2], m = params[4 * i + 3];
    W = 0;
    if (!t.take(m ? (pieces ? pieces[i] : nullptr) : nullptr, m)) return false;
    if (t.L == 0 || count == 0) return true;
    const unsigned __int128 all = (unsigned __int128)count * t.L, last = (unsigned __int128)offset + (unsigned __int128)(count - 1) * stride + t.given_end;
    if ((count > 1 && stride < t.given_end) || all > UINT64_MAX || last > UINT64_MAX) return false;
    W = (u64)all;
    return true;
}

// The three partial decode calls: the whole-call checks they share, frame i's request from make(i, request) (false: an invalid one, which fails
// the whole call before any write), then decompress_frames.  A base is device memory of the same GPU, and `out` is the base itself or does not
// overlap it; the overlap is judged on the w = min(out_sizes[i], base_sizes[i], what the request names) bytes the call can touch of each: two
// runs of w bytes overlap iff they start less than w apart.
int decompress_requests(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[], bool params_ok, const void * const bases[],
                        const size_t base_sizes[], void * const outs[], size_t out_sizes[], int rcs[],
                        const std::function<bool(s32, Request &)> & make) {
    if (n == 0) return BZ3_OK;
    std::vector<Request> reqs;
    int dev = -2;
    if (!request_front(n, elem_sizes, ins, in_sizes, params_ok && (!bases || base_sizes), outs, out_sizes, rcs, make, reqs, dev) || dev == -2)
        return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    for (s32 i = 0; bases && i < n; i++) {
        if (!bases[i] || !base_sizes[i]) continue;
        const u64 w = std::min<u64>({(u64)out_sizes[i], (u64)base_sizes[i], reqs[(size_t)i].wanted}), x = (u64)outs[i], y = (u64)bases[i];
        if (device_of(bases[i]) != dev || (x != y && (x > y ? x - y : y - x) < w)) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    }
    decompress_frames(dev, n, elem_sizes, (const u8 * const *)ins, in_sizes, (const u8 * const *)bases, base_sizes, (u8 * const *)outs, out_sizes, rcs, reqs.data());
    return first_error(n, rcs);
}
}  // namespace

BZIP3_API int bz3_hip_compress_device_delta(uint32_t block_size, uint32_t elem_size, const void * in, const void * base, void * out, size_t in_size,
                                            size_t * out_size) {
    if (!planes_elem_size_ok(elem_size)) return BZ3_ERR_INIT;
    const int dev = device_of(out);
    if (dev < 0 || (in_size && device_of(in) != dev)) return BZ3_ERR_INIT;
    if (base && in_size && (device_of(base) != dev || ranges_overlap(out, *out_size, base, in_size) || ranges_overlap(out, *out_size, in, in_size))) return BZ3_ERR_INIT;
    const u8 * ins[1] = {(const u8 *)in};
    const u8 * bases[1] = {(const u8 *)base};
    u8 * outs[1] = {(u8 *)out};
    int rc = BZ3_OK;
    compress_frames(dev, block_size, 1, &elem_size, ins, bases, &in_size, outs, out_size, &rc);
    return rc;
}

BZIP3_API int bz3_hip_compress_device_planes(uint32_t block_size, uint32_t elem_size, const void * in, void * out, size_t in_size, size_t * out_size) {
    return bz3_hip_compress_device_delta(block_size, elem_size, in, nullptr, out, in_size, out_size);
}

BZIP3_API int bz3_hip_compress_device(uint32_t block_size, const void * in, void * out, size_t in_size, size_t * out_size) {
    return bz3_hip_compress_device_planes(block_size, 1, in, out, in_size, out_size);
}

BZIP3_API int bz3_hip_decompress_device_delta(uint32_t elem_size, const void * in, const void * base, size_t base_size, void * out, size_t in_size,
                                              size_t * out_size) {
    if (!planes_elem_size_ok(elem_size)) return BZ3_ERR_INIT;
    if (in_size < 13) return BZ3_ERR_MALFORMED_HEADER;
    const int dev = device_of(in);
    if (dev < 0 || (*out_size && device_of(out) != dev)) return BZ3_ERR_INIT;
    if (base && base_size && (device_of(base) != dev || (base != out && ranges_overlap(out, *out_size, base, base_size)))) return BZ3_ERR_INIT;
    const u8 * ins[1] = {(const u8 *)in};
    const u8 * bases[1] = {(const u8 *)base};
    u8 * outs[1] = {(u8 *)out};
    int rc = BZ3_OK;
    decompress_frames(dev, 1, &elem_size, ins, &in_size, bases, &base_size, outs, out_size, &rc);
    return rc;
}

BZIP3_API int bz3_hip_decompress_device_planes(uint32_t elem_size, const void * in, void * out, size_t in_size, size_t * out_size) {
    return bz3_hip_decompress_device_delta(elem_size, in, nullptr, 0, out, in_size, out_size);
}

BZIP3_API int bz3_hip_decompress_device(const void * in, void * out, size_t in_size, size_t * out_size) {
    return bz3_hip_decompress_device_planes(1, in, out, in_size, out_size);
}

BZIP3_API int bz3_hip_frame_decoded_size_device(const void * in, size_t in_size, size_t * decoded_size) {
    *decoded_size = 0;
    if (in_size < 13) return BZ3_ERR_MALFORMED_HEADER;
    const int dev = device_of(in);
    if (dev < 0) return BZ3_ERR_INIT;
    const u8 * ins[1] = {(const u8 *)in};
    int rc = BZ3_OK;
    decoded_sizes_frames(dev, 1, ins, &in_size, decoded_size, &rc);
    return rc;
}

// (elem_sizes == NULL: element size 1 for every frame, as bz3_hip.h says; bases == NULL: no frame has a base.  The calls without _delta pass them.)
BZIP3_API int bz3_hip_compress_device_delta_many(uint32_t block_size, int32_t n, const uint32_t elem_sizes[], const void * const ins[], const void * const bases[],
                                                 const size_t in_sizes[], void * const outs[], size_t out_sizes[], int rcs[]) {
    if (n == 0) return BZ3_OK;
    if (n < 0 || !ins || !in_sizes || !outs || !out_sizes || !rcs) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    if (elem_sizes && !elem_sizes_ok(n, elem_sizes)) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    int dev = frames_device(n, ins, in_sizes, (const void * const *)outs, out_sizes);
    if (dev == -2) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    for (s32 i = 0; bases && i < n; i++) {  // a base: in_sizes[i] bytes of the same GPU that the frame's output overlaps neither with it nor with the input
        if (!bases[i] || !in_sizes[i]) continue;
        if (device_of(bases[i]) != dev || ranges_overlap(outs[i], out_sizes[i], bases[i], in_sizes[i]) || ranges_overlap(outs[i], out_sizes[i], ins[i], in_sizes[i]))
            return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    }
    compress_frames(dev, block_size, n, elem_sizes, (const u8 * const *)ins, (const u8 * const *)bases, in_sizes, (u8 * const *)outs, out_sizes, rcs);
    return first_error(n, rcs);
}

BZIP3_API int bz3_hip_compress_device_planes_many(uint32_t block_size, int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                  void * const outs[], size_t out_sizes[], int rcs[]) {
    return bz3_hip_compress_device_delta_many(block_size, n, elem_sizes, ins, nullptr, in_sizes, outs, out_sizes, rcs);
}

BZIP3_API int bz3_hip_compress_device_many(uint32_t block_size, int32_t n, const void * const ins[], const size_t in_sizes[], void * const outs[],
                                           size_t out_sizes[], int rcs[]) {
    return bz3_hip_compress_device_planes_many(block_size, n, nullptr, ins, in_sizes, outs, out_sizes, rcs);
}

BZIP3_API int bz3_hip_decompress_device_delta_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                   const void * const bases[], const size_t base_sizes[], void * const outs[], size_t out_sizes[], int rcs[]) {
    if (n == 0) return BZ3_OK;
    if (n < 0 || !ins || !in_sizes || !outs || !out_sizes || !rcs || (bases && !base_sizes)) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    if (elem_sizes && !elem_sizes_ok(n, elem_sizes)) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    const int dev = frames_device(n, ins, in_sizes, (const void * const *)outs, out_sizes);
    if (dev == -2) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    for (s32 i = 0; bases && i < n; i++) {  // a base: device memory of the same GPU; `out` is the base itself or does not overlap it
        if (!bases[i] || !base_sizes[i]) continue;
        if (device_of(bases[i]) != dev || (bases[i] != outs[i] && ranges_overlap(outs[i], out_sizes[i], bases[i], base_sizes[i])))
            return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    }
    decompress_frames(dev, n, elem_sizes, (const u8 * const *)ins, in_sizes, (const u8 * const *)bases, base_sizes, (u8 * const *)outs, out_sizes, rcs);
    return first_error(n, rcs);
}

BZIP3_API int bz3_hip_decompress_device_range_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                   const uint64_t offsets[], const void * const bases[], const size_t base_sizes[], void * const outs[],
                                                   size_t out_sizes[], int rcs[]) {
    return decompress_requests(n, elem_sizes, ins, in_sizes, true, bases, base_sizes, outs, out_sizes, rcs, [&](s32 i, Request & r) {
        r = Request::range(offsets ? offsets[i] : 0);
        return true;
    });
}

// params: per frame (offset, run, stride, count), valid as bz3_hip.h demands.
BZIP3_API int bz3_hip_decompress_device_strided_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                     const uint64_t params[], const void * const bases[], const size_t base_sizes[], void * const outs[],
                                                     size_t out_sizes[], int rcs[]) {
    return decompress_requests(n, elem_sizes, ins, in_sizes, params != nullptr, bases, base_sizes, outs, out_sizes, rcs, [&](s32 i, Request & r) {
        const u64 offset = params[4 * i], run = params[4 * i + 1], stride = params[4 * i + 2], count = params[4 * i + 3];
        if (run && count) {  // (else W = 0)
            const unsigned __int128 W = (unsigned __int128)count * run, last = (unsigned __int128)offset + (unsigned __int128)(count - 1) * stride + run;
            if ((count > 1 && stride < run) || W > UINT64_MAX || last > UINT64_MAX) return false;
        }
        r = Request::strided(offset, run, stride, count);
        return true;
    });
}

BZIP3_API int bz3_hip_decompress_device_strided(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, uint64_t run, uint64_t stride, uint64_t count,
                                                const void * base, size_t base_size, void * out, size_t * out_size) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    const uint64_t params[4] = {offset, run, stride, count};
    int rc = BZ3_OK;
    return bz3_hip_decompress_device_strided_many(1, &elem_size, ins, &in_size, params, bases, &base_size, outs, out_size, &rc);
}

// params: per frame (offset, stride, count, m); pieces[i]: m pairs (s_j, l_j) in host memory, valid as bz3_hip.h demands.  Request::select gives a
// request its normal form: no piece left is the empty request, one piece the strided request (offset + s_0, l_0, stride, count), so a call
// without a frame of two or more pieces is that strided call.
BZIP3_API int bz3_hip_decompress_device_select_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                                    const uint64_t params[], const uint64_t * const pieces[], const void * const bases[], const size_t base_sizes[],
                                                    void * const outs[], size_t out_sizes[], int rcs[]) {
    std::vector<PieceTable> tables;  // (sized once the whole-call checks have passed)
    return decompress_requests(n, elem_sizes, ins, in_sizes, params != nullptr, bases, base_sizes, outs, out_sizes, rcs, [&](s32 i, Request & r) {
        tables.resize((size_t)n);
        PieceTable & t = tables[(size_t)i];
        u64 W;
        if (!read_index_set(params, pieces, i, t, W)) return false;
        r = Request::select(params[4 * i], params[4 * i + 1], params[4 * i + 2], t);
        return true;
    });
}

BZIP3_API int bz3_hip_decompress_device_select(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, uint64_t stride, uint64_t count, uint64_t m,
                                               const uint64_t * pieces, const void * base, size_t base_size, void * out, size_t * out_size) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    const uint64_t params[4] = {offset, stride, count, m};
    const uint64_t * lists[1] = {pieces};
    int rc = BZ3_OK;
    return bz3_hip_decompress_device_select_many(1, &elem_size, ins, &in_size, params, lists, bases, &base_size, outs, out_size, &rc);
}

BZIP3_API int bz3_hip_decompress_device_range(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, const void * base, size_t base_size, void * out,
                                              size_t * out_size) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    int rc = BZ3_OK;
    return bz3_hip_decompress_device_range_many(1, &elem_size, ins, &in_size, &offset, bases, &base_size, outs, out_size, &rc);
}

// Range and index update (bz3_hip.h).  Whole-call checks as in the range calls; frame i's request from make(i, request) (false: an invalid one, which
// fails the whole call before any write); then, before any write, the overlaps of a frame's out[0, cap) with its input, its data and its base.
namespace {
int update_requests(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[], bool params_ok, const void * const datas[], const size_t ws[],
                    const void * const bases[], void * const outs[], size_t out_sizes[], int rcs[], const std::function<bool(s32, Request &)> & make) {
    if (n == 0) return BZ3_OK;
    std::vector<Request> reqs;
    int dev = -2;
    if (!request_front(n, elem_sizes, ins, in_sizes, params_ok && datas && ws, outs, out_sizes, rcs, make, reqs, dev) || dev < 0)
        return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);  // (dev == -1: every frame is empty and has no room: nothing to walk, nowhere to write)
    for (s32 i = 0; i < n; i++) {
        const void * base = bases ? bases[i] : nullptr;
        if (ws[i] && (device_of(datas[i]) != dev || (base && device_of(base) != dev))) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
        if (ranges_overlap(outs[i], out_sizes[i], ins[i], in_sizes[i]) || ranges_overlap(outs[i], out_sizes[i], datas[i], ws[i]) ||
            (base && ranges_overlap(outs[i], out_sizes[i], base, ws[i])))
            return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    }
    update_frames(dev, n, elem_sizes, (const u8 * const *)ins, in_sizes, reqs.data(), (const u8 * const *)datas, ws, (const u8 * const *)bases, (u8 * const *)outs, out_sizes, rcs);
    return first_error(n, rcs);
}
}  // namespace

BZIP3_API int bz3_hip_update_device_range_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[], const uint64_t offsets[],
                                               const void * const datas[], const size_t ws[], const void * const bases[], void * const outs[], size_t out_sizes[],
                                               int rcs[]) {
    return update_requests(n, elem_sizes, ins, in_sizes, true, datas, ws, bases, outs, out_sizes, rcs, [&](s32 i, Request & r) {
        r = Request::range(offsets ? offsets[i] : 0);
        return true;
    });
}

// params: per frame (offset, stride, count, m); pieces[i]: m pairs (s_j, l_j) in host memory, valid as the index decode demands; ws[i] must be
// W = count L.  The normal form: no byte named is the empty range (offset is not looked at); one piece left with count == 1 or stride == L is the
// range (offset + s_0, W), which takes the range update's path bit for bit; everything else patches with its piece table, one piece included (a
// strided update is the one-piece table: planes.hpp has no strided split).
BZIP3_API int bz3_hip_update_device_select_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[], const uint64_t params[],
                                                const uint64_t * const pieces[], const void * const datas[], const size_t ws[], const void * const bases[],
                                                void * const outs[], size_t out_sizes[], int rcs[]) {
    std::vector<PieceTable> tables;  // (sized once the whole-call checks have passed)
    return update_requests(n, elem_sizes, ins, in_sizes, params != nullptr, datas, ws, bases, outs, out_sizes, rcs, [&](s32 i, Request & r) {
        const u64 offset = params[4 * i], stride = params[4 * i + 1], count = params[4 * i + 2];
        tables.resize((size_t)n);
        PieceTable & t = tables[(size_t)i];
        u64 W;
        if (!read_index_set(params, pieces, i, t, W) || W != (u64)ws[i]) return false;
        if (W == 0) {  // the verbatim copy
            r = Request::range(0);
            return true;
        }
        if (t.m == 1 && (count == 1 || stride == t.L)) {
            r = Request::range(offset + t.s(0));
        } else {
            r = Request::strided(offset, t.L, stride, count);
            r.sel = &t;
        }
        return true;
    });
}

BZIP3_API int bz3_hip_update_device_select(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, uint64_t stride, uint64_t count, uint64_t m,
                                           const uint64_t * pieces, const void * data, size_t w, const void * base, void * out, size_t * out_size) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * datas[1] = {data};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    const uint64_t params[4] = {offset, stride, count, m};
    const uint64_t * lists[1] = {pieces};
    int rc = BZ3_OK;
    return bz3_hip_update_device_select_many(1, &elem_size, ins, &in_size, params, lists, datas, &w, bases, outs, out_size, &rc);
}

BZIP3_API int bz3_hip_update_device_range(uint32_t elem_size, const void * in, size_t in_size, uint64_t offset, const void * data, size_t w, const void * base, void * out,
                                          size_t * out_size) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * datas[1] = {data};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    int rc = BZ3_OK;
    return bz3_hip_update_device_range_many(1, &elem_size, ins, &in_size, &offset, datas, &w, bases, outs, out_size, &rc);
}

// Sync (bz3_hip.h).  The whole-call checks of the update calls, with `old` beside `data`: both are device memory of the call's GPU wherever
// sizes[i] > 0, and a frame's out[0, cap) overlaps none of its input, its data, its old and its base.  Then update_frames in its sync mode.
BZIP3_API int bz3_hip_sync_device_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[], const void * const datas[],
                                       const void * const olds[], const size_t sizes[], const void * const bases[], void * const outs[], size_t out_sizes[],
                                       uint32_t recoded[], int rcs[]) {
    if (n == 0) return BZ3_OK;
    for (s32 i = 0; recoded && i < n; i++) recoded[i] = 0;
    std::vector<Request> reqs;
    int dev = -2;
    if (!request_front(n, elem_sizes, ins, in_sizes, datas && olds && sizes, outs, out_sizes, rcs, [](s32, Request & r) { return r = Request::range(0), true; }, reqs, dev) ||
        dev < 0)
        return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);  // (dev == -1: every frame is empty and has no room: nothing to walk, nowhere to write)
    for (s32 i = 0; i < n; i++) {
        const void * base = bases ? bases[i] : nullptr;
        if (sizes[i] && (device_of(datas[i]) != dev || device_of(olds[i]) != dev || (base && device_of(base) != dev))) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
        if (ranges_overlap(outs[i], out_sizes[i], ins[i], in_sizes[i]) || ranges_overlap(outs[i], out_sizes[i], datas[i], sizes[i]) ||
            ranges_overlap(outs[i], out_sizes[i], olds[i], sizes[i]) || (base && ranges_overlap(outs[i], out_sizes[i], base, sizes[i])))
            return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    }
    update_frames(dev, n, elem_sizes, (const u8 * const *)ins, in_sizes, reqs.data(), (const u8 * const *)datas, sizes, (const u8 * const *)bases, (u8 * const *)outs, out_sizes,
                  rcs, (const u8 * const *)olds, recoded);
    return first_error(n, rcs);
}

BZIP3_API int bz3_hip_sync_device(uint32_t elem_size, const void * in, size_t in_size, const void * data, const void * old, size_t size, const void * base, void * out,
                                  size_t * out_size, uint32_t * recoded) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * datas[1] = {data};
    const void * olds[1] = {old};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    int rc = BZ3_OK;
    return bz3_hip_sync_device_many(1, &elem_size, ins, &in_size, datas, olds, &size, bases, outs, out_size, recoded, &rc);
}

// Resize (bz3_hip.h).  The whole-call checks of the update calls, the overlaps of a frame's out[0, cap) with its input, its data and its base, then
// resize_frames.
BZIP3_API int bz3_hip_resize_device_many(int32_t n, const uint32_t block_sizes[], const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[],
                                         const uint64_t keeps[], const void * const datas[], const size_t ws[], const void * const bases[], void * const outs[],
                                         size_t out_sizes[], int rcs[]) {
    if (n == 0) return BZ3_OK;
    if (n < 0 || !block_sizes || !ins || !in_sizes || !keeps || !datas || !ws || !outs || !out_sizes || !rcs || (elem_sizes && !elem_sizes_ok(n, elem_sizes)))
        return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    const int dev = frames_device(n, ins, in_sizes, (const void * const *)outs, out_sizes);
    if (dev < 0) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);  // (dev == -1: every frame is empty and has no room: nothing to walk, nowhere to write)
    for (s32 i = 0; i < n; i++) {
        const void * base = bases ? bases[i] : nullptr;
        if (ws[i] && (device_of(datas[i]) != dev || (base && device_of(base) != dev))) return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
        if (ranges_overlap(outs[i], out_sizes[i], ins[i], in_sizes[i]) || ranges_overlap(outs[i], out_sizes[i], datas[i], ws[i]) ||
            (base && ranges_overlap(outs[i], out_sizes[i], base, ws[i])))
            return fail_frames(n, rcs, out_sizes, BZ3_ERR_INIT);
    }
    resize_frames(dev, n, block_sizes, elem_sizes, (const u8 * const *)ins, in_sizes, keeps, (const u8 * const *)datas, ws, (const u8 * const *)bases, (u8 * const *)outs,
                  out_sizes, rcs);
    return first_error(n, rcs);
}

BZIP3_API int bz3_hip_resize_device(uint32_t block_size, uint32_t elem_size, const void * in, size_t in_size, uint64_t keep, const void * data, size_t w,
                                    const void * base, void * out, size_t * out_size) {
    if (!out_size) return BZ3_ERR_INIT;
    const void * ins[1] = {in};
    const void * datas[1] = {data};
    const void * bases[1] = {base};
    void * outs[1] = {out};
    int rc = BZ3_OK;
    return bz3_hip_resize_device_many(1, &block_size, &elem_size, ins, &in_size, &keep, datas, &w, bases, outs, out_size, &rc);
}

BZIP3_API int bz3_hip_decompress_device_planes_many(int32_t n, const uint32_t elem_sizes[], const void * const ins[], const size_t in_sizes[], void * const outs[],
                                                    size_t out_sizes[], int rcs[]) {
    return bz3_hip_decompress_device_delta_many(n, elem_sizes, ins, in_sizes, nullptr, nullptr, outs, out_sizes, rcs);
}

BZIP3_API int bz3_hip_decompress_device_many(int32_t n, const void * const ins[], const size_t in_sizes[], void * const outs[], size_t out_sizes[],
                                             int rcs[]) {
    return bz3_hip_decompress_device_planes_many(n, nullptr, ins, in_sizes, outs, out_sizes, rcs);
}

BZIP3_API int bz3_hip_frame_decoded_sizes_device(int32_t n, const void * const ins[], const size_t in_sizes[], size_t decoded_sizes[], int rcs[]) {
    if (n == 0) return BZ3_OK;
    if (n < 0 || !ins || !in_sizes || !decoded_sizes || !rcs) return fail_frames(n, rcs, decoded_sizes, BZ3_ERR_INIT);
    const int dev = frames_device(n, ins, in_sizes, nullptr, nullptr);
    if (dev == -2) return fail_frames(n, rcs, decoded_sizes, BZ3_ERR_INIT);
    decoded_sizes_frames(dev, n, (const u8 * const *)ins, in_sizes, decoded_sizes, rcs);
    return first_error(n, rcs);
}

namespace {
// What a single-shot call owns: a non-blocking stream and one device allocation on the current device.  However the call ends, the
// stream is waited for, then the allocation freed, then the stream destroyed.
struct ScratchStream {
    hipStream_t s = nullptr;
    u8 * mem = nullptr;
    ScratchStream() = default;
    ScratchStream(const ScratchStream &) = delete;
    ScratchStream & operator=(const ScratchStream &) = delete;
    void open(size_t bytes) {
        HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP_CHECK(hipMalloc((void **)&mem, bytes));
    }
    ~ScratchStream() {
        if (s) (void)hipStreamSynchronize(s);
        if (mem) (void)hipFree(mem);
        if (s) (void)hipStreamDestroy(s);
    }
};

// The frame of a debug launch: dst, src and (with need_base) base are device memory of one GPU; then a stream and an allocation for the tables of
// n segments up to `level` and `extra` bytes behind them, the segments from fill(g, the device address of the extra bytes, the stream), one
// launch.  BZ3_ERR_INIT for everything that goes wrong.
int32_t debug_launch(const void * src, const void * base, bool need_base, void * dst, size_t n, int level, size_t extra,
                     const std::function<void(GatherList &, u8 *, hipStream_t)> & fill) {
    const int dev = device_of(dst);
    if (dev < 0 || device_of(src) != dev || (need_base && device_of(base) != dev)) return BZ3_ERR_INIT;
    ScratchStream sc;
    try {
        DeviceGuard g(dev);
        const size_t tab_bytes = align256(table_bytes(n, level));
        sc.open(tab_bytes + extra);
        GatherList list;
        fill(list, sc.mem + tab_bytes, sc.s);
        std::vector<u8> staging;
        copy_segments(list, staging, sc.mem, sc.s);
        HIP_CHECK(hipStreamSynchronize(sc.s));
    } catch (...) {
        return BZ3_ERR_INIT;
    }
    return BZ3_OK;
}

// n segments of `width` u64 each relative to src / base / dst, one launch: (src_off, dst_off, len[, elem_size | inverse << 8]), or with
// width 5 (src_off, base_off, dst_off, len, elem_size | inverse << 8), base_off = UINT64_MAX for a segment without a base.
int32_t debug_move_segments(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n, int width) {
    if (n < 0 || (n > 0 && !segs)) return BZ3_ERR_INIT;
    for (s32 i = 0; width >= 4 && i < n; i++) {
        const u64 mode = segs[width * i + width - 1];
        if (!planes_elem_size_ok(mode & 0xff) || (mode >> 9)) return BZ3_ERR_INIT;
    }
    return debug_launch(src, base, width == 5, dst, (size_t)n, SEG_DELTA, 0, [&](GatherList & g, u8 *, hipStream_t) {
        for (s32 i = 0; i < n; i++) {
            const uint64_t * q = segs + (size_t)width * i;
            if (width == 5) g.plain({(u64)src + q[0], (u64)dst + q[2], q[3], q[4], q[1] == UINT64_MAX ? 0 : (u64)base + q[1]});
            else g.plain({(u64)src + q[0], (u64)dst + q[1], q[2], width == 4 ? q[3] : 0, 0});
        }
    });
}

// The base address of a debug tuple's segment: base_off == UINT64_MAX is no base.
u64 debug_base(const void * base, u64 base_off) { return base_off == UINT64_MAX ? 0 : (u64)base + base_off; }

// The body of bz3_hip_debug_range and bz3_hip_debug_patch: n septuples whose fifth field must be elem_size | mode_bits << 8 and whose [a, b) must lie
// in their len bytes, one launch of the segments add(list, septuple) makes of them.
int32_t debug_clips(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n, u64 mode_bits, const std::function<void(GatherList &, const uint64_t *)> & add) {
    if (n < 0 || (n > 0 && !segs)) return BZ3_ERR_INIT;
    bool any_base = false;
    for (s32 i = 0; i < n; i++) {
        const uint64_t * q = segs + (size_t)7 * i;
        if (!planes_elem_size_ok(q[4] & 0xff) || (q[4] >> 8) != mode_bits || q[5] > q[6] || q[6] > q[3]) return BZ3_ERR_INIT;
        any_base |= q[1] != UINT64_MAX;
    }
    return debug_launch(src, base, any_base, dst, (size_t)n, SEG_CLIP, 0, [&](GatherList & g, u8 *, hipStream_t) {
        for (s32 i = 0; i < n; i++) add(g, segs + (size_t)7 * i);
    });
}
}  // namespace

BZIP3_API int32_t bz3_hip_debug_copy_segments(const void * src, void * dst, const uint64_t * segs, int32_t n) { return debug_move_segments(src, nullptr, dst, segs, n, 3); }

BZIP3_API int32_t bz3_hip_debug_planes(const void * src, void * dst, const uint64_t * segs, int32_t n) { return debug_move_segments(src, nullptr, dst, segs, n, 4); }

// n triples (a_off, b_off, len) relative to a / b: flags[i] = 1 iff a[a_off, a_off + len) and b[b_off, b_off + len) differ, else 0, one launch of
// k_diff_segments through the table a sync call's walk round makes (diff_segments).
BZIP3_API int32_t bz3_hip_debug_diff(const void * a, const void * b, const uint64_t * segs, int32_t n, uint32_t * flags) {
    if (n < 0 || (n > 0 && (!segs || !flags))) return BZ3_ERR_INIT;
    if (n == 0) return BZ3_OK;
    const int dev = device_of(a);
    if (dev < 0 || device_of(b) != dev) return BZ3_ERR_INIT;
    ScratchStream sc;
    try {
        DeviceGuard g(dev);
        const size_t tab_bytes = align256(table_bytes((size_t)n, SEG_DELTA));
        sc.open(tab_bytes + (size_t)n * sizeof(u32));
        std::vector<CopySeg> v;
        for (s32 i = 0; i < n; i++) v.push_back({(u64)a + segs[3 * i], 0, segs[3 * i + 2], (u64)i, (u64)b + segs[3 * i + 1]});
        std::vector<u8> staging;
        diff_segments(v, staging, sc.mem, (u32 *)(sc.mem + tab_bytes), flags, (size_t)n, sc.s);
    } catch (...) {
        return BZ3_ERR_INIT;
    }
    return BZ3_OK;
}

BZIP3_API int32_t bz3_hip_debug_delta(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n) {
    return debug_move_segments(src, base, dst, segs, n, 5);
}

// n septuples (src_off, base_off, dst_off, len, elem_size | 1 << 8, a, b): of the merge of the `len` bytes at src_off the bytes [a, b), to
// dst_off (plus the bytes at base_off unless it is UINT64_MAX), one launch through the segments a range call's gather makes of them.
BZIP3_API int32_t bz3_hip_debug_range(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n) {
    return debug_clips(src, base, dst, segs, n, 1, [&](GatherList & g, const uint64_t * q) {
        g.range((u64)src + q[0], q[3], q[4] & 0xff, q[5], q[6], (u64)dst + q[2], debug_base(base, q[1]));
    });
}

// n septuples (src_off, base_off, dst_off, len, elem_size, a, b): the slot of `len` bytes at dst_off holds a chunk in split form, of which the bytes
// [a, b) get the values at src_off (less the bytes at base_off unless it is UINT64_MAX), one launch through the segments an update call's patch
// makes of them.
BZIP3_API int32_t bz3_hip_debug_patch(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n) {
    return debug_clips(src, base, dst, segs, n, 0, [&](GatherList & g, const uint64_t * q) {
        g.patch((u64)src + q[0], debug_base(base, q[1]), (u64)dst + q[2], q[3], q[4], q[5], q[6]);
    });
}

// n sextuples (src_off, dst_off, len_old, len_new, elem_size, a): the slot of len_old bytes at src_off holds a chunk in split form, whose bytes
// [0, a) go to where the slot of len_new bytes at dst_off keeps them, one launch through the segments a resize call's patch makes of them.
BZIP3_API int32_t bz3_hip_debug_replane(const void * src, void * dst, const uint64_t * segs, int32_t n) {
    if (n < 0 || (n > 0 && !segs)) return BZ3_ERR_INIT;
    for (s32 i = 0; i < n; i++) {
        const uint64_t * q = segs + (size_t)6 * i;
        if (!planes_elem_size_ok(q[4]) || q[5] > q[2] || q[5] > q[3]) return BZ3_ERR_INIT;
    }
    return debug_launch(src, nullptr, false, dst, (size_t)n, SEG_CLIP, 0, [&](GatherList & g, u8 *, hipStream_t) {
        for (s32 i = 0; i < n; i++) {
            const uint64_t * q = segs + (size_t)6 * i;
            g.replane((u64)src + q[0], (u64)dst + q[1], q[2], q[3], q[4], q[5]);
        }
    });
}

// n tuples of 10 u64 (src_off, base_off, dst_off, len, elem_size | 1 << 8, c0, first, run, stride, nbytes): of the merge of the `len` bytes at
// src_off the nbytes bytes c(u) (planes.hpp, "Strided merge"), to dst_off (plus the bytes at base_off unless it is UINT64_MAX), one launch through
// the segments a strided call's gather makes of them.  stride == run is not normalised away here: it reaches the kernel.
BZIP3_API int32_t bz3_hip_debug_strided(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n) {
    if (n < 0 || (n > 0 && !segs)) return BZ3_ERR_INIT;
    bool any_base = false;
    for (s32 i = 0; i < n; i++) {
        const uint64_t * q = segs + (size_t)10 * i;
        if (!planes_elem_size_ok(q[4] & 0xff) || (q[4] >> 8) != 1 || q[3] >= ((u64)1 << 31)) return BZ3_ERR_INIT;
        if (q[9] && (q[7] == 0 || q[6] == 0 || q[6] > q[7] || q[8] < q[7] || strided_last_byte(q[5], q[6], q[7], q[8], q[9]) >= q[3])) return BZ3_ERR_INIT;
        any_base |= q[1] != UINT64_MAX;
    }
    return debug_launch(src, base, any_base, dst, (size_t)n, SEG_STRIDED, 0, [&](GatherList & g, u8 *, hipStream_t) {
        for (s32 i = 0; i < n; i++) {
            const uint64_t * q = segs + (size_t)10 * i;
            g.strided((u64)src + q[0], q[3], q[4] & 0xff, q[9] ? q[5] : 0, q[6], q[7], q[8], q[9], (u64)dst + q[2], debug_base(base, q[1]));
        }
    });
}

namespace {
// The checks the two select hooks share on their n tuples of 12 u64, whose fifth field must be elem_size | mode_bits: the tables of the tuples as
// they are given (tabs), one after the other as they are uploaded (all), and whether a tuple has a base.  False for what bz3_hip.h refuses.
bool debug_select_tuples(const uint64_t * segs, int32_t n, const uint64_t * pieces, uint64_t n_pieces, u64 mode_bits, std::vector<PieceTable> & tabs, std::vector<u64> & all,
                         bool & any_base) {
    if (n < 0 || (n > 0 && !segs) || (n_pieces && !pieces)) return false;
    tabs.resize((size_t)std::max(n, 0));
    for (s32 i = 0; i < n; i++) {
        const uint64_t * q = segs + (size_t)12 * i;
        const u64 len = q[3], rel = q[5], stride = q[6], q0 = q[7], r0 = q[8], nbytes = q[9], first = q[10], m = q[11];
        if (!planes_elem_size_ok(q[4] & 0xff) || (q[4] >> 8) != mode_bits || len >= ((u64)1 << 31) || nbytes > len) return false;
        if (first > n_pieces || m > n_pieces - first || m >= ((u64)1 << 31)) return false;
        PieceTable & t = tabs[(size_t)i];
        if (!t.take(m ? pieces + 2 * first : nullptr, m, false)) return false;
        all.insert(all.end(), t.tab.begin(), t.tab.end());
        any_base |= q[1] != UINT64_MAX;
        if (!nbytes) continue;
        if (t.L == 0 || r0 >= t.L || (nbytes > t.L - r0 && stride < t.given_end)) return false;
        for (const u64 u : {(u64)0, nbytes - 1}) {  // c(0) and c(nbytes - 1) lie in the chunk (c increases)
            const u64 x = r0 + u;
            const unsigned __int128 period = (unsigned __int128)q0 + x / t.L;
            if (stride && period > UINT64_MAX / stride) return false;
            const __int128 c = (__int128)(s64)rel + (__int128)(period * stride) + t.byte(x % t.L);
            if (c < 0 || c >= (__int128)len) return false;
        }
    }
    return true;
}

// The body of the two select hooks: those checks, the tables uploaded behind the launch's own, and one launch of the segments that
// add(list, tuple, its table, the table's device address) makes of the tuples that name a byte.
int32_t debug_selects(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n, const uint64_t * pieces, uint64_t n_pieces, u64 mode_bits,
                      const std::function<void(GatherList &, const uint64_t *, const PieceTable &, u64)> & add) {
    bool any_base = false;
    std::vector<PieceTable> tabs;
    std::vector<u64> all;
    if (!debug_select_tuples(segs, n, pieces, n_pieces, mode_bits, tabs, all, any_base)) return BZ3_ERR_INIT;
    return debug_launch(src, base, any_base, dst, (size_t)n, SEG_SELECT, all.size() * sizeof(u64) + 16, [&](GatherList & g, u8 * d_tabs, hipStream_t s) {
        if (!all.empty()) HIP_CHECK(hipMemcpyAsync(d_tabs, all.data(), all.size() * sizeof(u64), hipMemcpyHostToDevice, s));
        size_t at = 0;
        for (s32 i = 0; i < n; i++) {
            const uint64_t * q = segs + (size_t)12 * i;
            if (q[9]) add(g, q, tabs[(size_t)i], (u64)d_tabs + at * sizeof(u64));
            at += tabs[(size_t)i].tab.size();
        }
    });
}
}  // namespace

// n tuples of 12 u64 (src_off, base_off, dst_off, len, elem_size | 1 << 8, rel, stride, q0, r0, nbytes, first_piece, m): of the merge of the `len`
// bytes at src_off the nbytes bytes c(u) (planes.hpp, "Select merge") of the m pieces (s_j, l_j) from pieces[2 first_piece] on, to dst_off (plus the
// bytes at base_off unless it is UINT64_MAX), one launch through the segments a select call's gather makes of them.  The pieces are taken as they
// are, empty ones and neighbours that touch included.
BZIP3_API int32_t bz3_hip_debug_select(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n, const uint64_t * pieces, uint64_t n_pieces) {
    return debug_selects(src, base, dst, segs, n, pieces, n_pieces, 1, [&](GatherList & g, const uint64_t * q, const PieceTable & t, u64 d_tab) {
        g.select((u64)src + q[0], q[3], q[4] & 0xff, q[5], q[6], t, d_tab, q[7], q[8], q[9], (u64)dst + q[2], debug_base(base, q[1]));
    });
}

// bz3_hip_debug_select in the forward direction: n tuples of 12 u64 (src_off, base_off, dst_off, len, elem_size, rel, stride, q0, r0, nbytes, first_piece,
// m).  The slot of `len` bytes at dst_off holds a chunk in split form, of which the nbytes bytes c(u) (planes.hpp, "Select split") of the m pieces
// from pieces[2 first_piece] on get the values at src_off (less the bytes at base_off unless it is UINT64_MAX), one launch through the segments an
// update call's patch makes of them.  The pieces are taken as they are, empty ones and neighbours that touch included.
BZIP3_API int32_t bz3_hip_debug_patch_select(const void * src, const void * base, void * dst, const uint64_t * segs, int32_t n, const uint64_t * pieces, uint64_t n_pieces) {
    return debug_selects(src, base, dst, segs, n, pieces, n_pieces, 0, [&](GatherList & g, const uint64_t * q, const PieceTable & t, u64 d_tab) {
        g.patch_select((u64)src + q[0], debug_base(base, q[1]), (u64)dst + q[2], q[3], q[4], q[5], q[6], t, d_tab, q[7], q[8], q[9]);
    });
}

// The CRC-32C of bz3's block headers (crc32sum, src/libbz3.c: state init, no inversion) of n buffers in device memory of one GPU, at any
// alignment: crc32c_device_many (crc32c.hip) on the callers' buffers.  Per call one stream, one allocation (the table, then the n result
// words), one table upload, one memset, at most two launches and one read-back, whatever n is.
BZIP3_API int bz3_hip_crc32c_device_many(int32_t n, const void * const * ptrs, const size_t * sizes, const uint32_t * inits, uint32_t * crcs) {
    if (n < 0 || (n > 0 && (!ptrs || !sizes || !crcs))) return BZ3_ERR_INIT;
    if (n == 0) return BZ3_OK;
    int dev = -1;
    u64 total_seg = 0;
    std::vector<CrcBuf> tab((size_t)n);
    for (s32 i = 0; i < n; i++) {
        tab[(size_t)i] = {sizes[i] ? dev_addr(ptrs[i]) : 0, (u64)sizes[i], inits ? inits[i] : 1u, (u32)total_seg};
        if (!sizes[i]) continue;
        const int d = device_of(ptrs[i]);
        if (d < 0 || (dev >= 0 && d != dev)) return BZ3_ERR_INIT;
        dev = d;
        total_seg += crc_many_segments(ptrs[i], (u64)sizes[i]);
        if (total_seg >= ((u64)1 << 31)) return BZ3_ERR_INIT;  // 32 TiB in one call
    }
    if (dev < 0) {  // nothing but empty buffers: no GPU is needed
        for (s32 i = 0; i < n; i++) crcs[i] = tab[(size_t)i].init;
        return BZ3_OK;
    }
    DeviceCtx * ctx = nullptr;
    try {
        ctx = get_ctx(dev);
    } catch (...) {
        ctx = nullptr;
    }
    if (!ctx) return BZ3_ERR_INIT;
    ScratchStream sc;
    int rc = BZ3_OK;
    try {
        DeviceGuard g(dev);
        const size_t tab_bytes = align256((size_t)n * sizeof(CrcBuf));
        std::vector<u32> got((size_t)n);
        sc.open(tab_bytes + (size_t)n * sizeof(u32));
        HIP_CHECK(hipMemcpyAsync(sc.mem, tab.data(), (size_t)n * sizeof(CrcBuf), hipMemcpyHostToDevice, sc.s));
        g_crc_launches += crc32c_device_many((const CrcBuf *)sc.mem, (u32)n, (u32)total_seg, ctx->d_crc, (u32 *)(sc.mem + tab_bytes), sc.s);
        HIP_CHECK(hipMemcpyAsync(got.data(), sc.mem + tab_bytes, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost, sc.s));
        HIP_CHECK(hipStreamSynchronize(sc.s));
        memcpy(crcs, got.data(), (size_t)n * sizeof(u32));  // nothing is written unless the whole call succeeded
    } catch (...) {
        rc = BZ3_ERR_INIT;
    }
    return rc;
}

BZIP3_API unsigned bz3_hip_debug_crc_launches(int reset) { return reset ? g_crc_launches.exchange(0) : g_crc_launches.load(); }

// One buffer: the n = 1 case of the call above.
BZIP3_API int bz3_hip_crc32c_device(const void * p, size_t n, uint32_t init, uint32_t * crc) {
    return bz3_hip_crc32c_device_many(1, &p, &n, &init, crc);
}

}  // extern "C"
