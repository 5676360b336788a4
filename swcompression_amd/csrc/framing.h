// framing.h -- host-side framing helpers shared between the C-ABI translation units.
#ifndef SWC_FRAMING_H
#define SWC_FRAMING_H
#include <memory>
#include <vector>
#include "host_util.h"
namespace swc {
struct GzipHeaderInfo { uint32_t bgzf_bsize; };
struct BlockRef64 { uint64_t offset, comp_len, uncomp_len; uint32_t aux; uint32_t flags = 0; };

// ---- streams through the engine as runs of units (framing_runs.cpp) ------------------------------------------------------------
// What one codec adds to run_streams: where its streams may be cut (Deflate: behind flush markers, framing_deflate.cpp; LZMA2: in
// front of dictionary resets, framing_lzma.cpp), what a unit needs, and when the units' result stands.
struct RunCodec {
    int codec;
    Stat fallbacks;            // counts the streams decoded whole after their units
    unsigned sums;             // bit k: the units' check sums of swc_checksum kind k combine into the stream's (CRC-32, Adler-32)
    size_t (*least_bytes)();   // the knob: the least compressed size of a unit, 0 = never cut
    // the units of a stream longer than the knob, without dictionary, not part of a chain; fewer than two: it stays whole
    void (*index)(const HostUnit& st, size_t least_bytes, std::vector<BlockRef64>& refs);
    // run[k] is unit_of(st, refs[k]): the rest of it -- room, place, check sum.  `again`: the same units as the launch left them, if
    // the run goes `once_more`.  `joined` is the run's own buffer for units that have no place in st.dst
    void (*fill)(const HostUnit& st, const std::vector<BlockRef64>& refs, HostUnit* run, const HostUnit* again, std::vector<uint8_t>& joined);
    bool (*once_more)(const HostUnit* run);   // nullptr: never
    // true: the units' result stands, run[last] is the unit that met the end of the stream, and st holds the output
    bool (*verdict)(HostUnit& st, const std::vector<BlockRef64>& refs, HostUnit* run, std::vector<uint8_t>& joined, size_t& last);
};
const RunCodec& deflate_runs();   // framing_deflate.cpp
const RunCodec& lzma2_runs();     // framing_lzma.cpp
HostUnit unit_of(const HostUnit& st, const BlockRef64& ref);   // a sub-range of the stream, which is staged once
// What run_units(codec, streams) would leave in every stream.  kCut: Deflate and LZMA2 streams go as runs of parallel units where
// they can be cut, in one launch wherever no stream has to fall back
enum Cut { kWhole, kCut };
int run_streams(int codec, std::vector<HostUnit>& streams, Cut cut);
int run_one(int codec, HostUnit& u, Cut cut = kWhole);
int run_one_bounded(int codec, HostUnit& u, size_t bound, Cut cut);
void give(const std::vector<uint8_t>& src, uint8_t** out, size_t* out_len);
void give_empty(uint8_t** out, size_t* out_len);
size_t* give_sizes(const std::vector<size_t>& v);
int gzip_parse_header(const uint8_t* d, size_t n, size_t& pos, GzipHeaderInfo* info);
int gzip_member_prepare(const uint8_t* d, size_t n, size_t pos, HostUnit& u);
int gzip_member_finish(const uint8_t* d, size_t n, size_t data_pos, const HostUnit& u, size_t& next_pos, bool& crc_error);
int zlib_parse_header(const uint8_t* d, size_t n, size_t& pos);
void set_deflate_unit_bytes(int v);   // "deflate_unit_bytes" (swc_set_tuning)
void set_deflate_units_linked(int v); // "deflate_units_linked" (swc_set_tuning)
void set_lzma2_run_bytes(int v);      // "lzma2_run_bytes" (swc_set_tuning)
void set_gzip_member_scan(int v);     // "gzip_member_scan" (swc_set_tuning)
void set_bzip2_scan_bytes(int v);     // "bzip2_scan_bytes" (swc_set_tuning)
void set_bgzf_round_members(int v);   // "bgzf_round_members" (swc_set_tuning): members per round of swc_bgzf_archive
// many-archive batching helpers (framing_many.cpp)
struct Lz4Plan {
    struct Impl;
    Impl* impl;
    int early_status = SWC_OK;
    size_t first_unit = 0;
    Lz4Plan();
    ~Lz4Plan();
    Lz4Plan(const Lz4Plan&) = delete;
    Lz4Plan& operator=(const Lz4Plan&) = delete;
};
bool lz4_plan_prepare(const uint8_t* in, size_t n, Lz4Plan& plan, std::vector<HostUnit>& units);
int lz4_plan_finish(const uint8_t* in, size_t n, const Lz4Plan& plan, const std::vector<HostUnit>& units, std::vector<uint8_t>& res);
// the copies in HBM of the archives whose marks the device found ("bzip2_scan_bytes"): the units of bzip2_collect_candidates address
// them (HostUnit::base_dev), so one of these outlives the run_units call that decodes them
struct Bzip2Staged { std::vector<std::unique_ptr<DevBuf>> files; };
void bzip2_collect_candidates(const uint8_t* d, size_t n, std::vector<HostUnit>& units, std::vector<uint64_t>& used, Bzip2Staged& keep);
int bzip2_finish_stream(const uint8_t* d, size_t n, std::vector<HostUnit>& units, size_t first_unit, const std::vector<uint64_t>& used,
                        std::vector<uint8_t>& res, size_t& byte_pos);
size_t lzma2_announced_size(const uint8_t* p, size_t n);
void set_sha256_device_min_units(int v);   // "sha256_device_min_units" (swc_set_tuning)
// XZArchive.unarchive of every archive of a set (framing_lzma.cpp): the blocks the indexes of ALL archives list decoded ahead in one
// launch, then every archive walked on its own.  statuses[i] / outs[i] as swc_xz_unarchive leaves them; SWC_OK or SWC_E_DEVICE.
int xz_run_many(const uint8_t* const* archives, const size_t* lens, size_t n, std::vector<int>& statuses, std::vector<std::vector<uint8_t>>& outs);
// block discovery for swc_index_blocks (framing_many.cpp)
bool bgzf_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
void gzip_member_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
void deflate_unit_index(const uint8_t* in, size_t in_len, size_t unit_bytes, std::vector<BlockRef64>& out);
size_t deflate_unit_bytes();
bool lz4_frame_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
void bzip2_magic_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
void bzip2_mark_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
void xz_block_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
int lzma2_chunk_index(const uint8_t* in, size_t in_len, std::vector<BlockRef64>& out);
int lzma2_chunk_walk(const uint8_t* in, size_t in_len, size_t p, std::vector<BlockRef64>& out);
void lzma2_unit_index(const uint8_t* in, size_t in_len, size_t first, uint8_t dict_byte, size_t run_bytes, std::vector<BlockRef64>& out);
size_t lzma2_run_bytes();
}
#endif
