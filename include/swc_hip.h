/*
 * swc_hip.h -- C ABI of libswc_hip.so, the MI355X (gfx950) many-stream decode engine that sits behind
 * SWCompression's `decompress(data:)` entry points.
 *
 * The reference (tsolomko/SWCompression 4.9.0) is pure Swift and has no FFI layer; its boundary for
 * this path is the protocol `DecompressionAlgorithm { static func decompress(data: Data) throws -> Data }`
 * (Sources/Common/DecompressionAlgorithm.swift:9-14) plus the internal reader-taking overloads that
 * the archive/container layers call.  Each entry point below names the Swift function whose BODY it
 * replaces (file:line under /root/reference); INTEGRATION.md shows the Swift-side binding.
 *
 * Rules common to all entry points
 *  - return value / swc_job.status is an swc_status (swc_status.h): 0 = OK, otherwise 1:1 with the Swift
 *    error enum case the reference would throw, SWC_E_REF_TRAP where the reference would trap.
 *  - single-shot calls take HOST buffers, run the HIP kernels (there is no CPU fallback: without a
 *    usable gfx950 device they return SWC_E_DEVICE), and hand back a malloc()ed buffer the caller
 *    releases with swc_free().  *out is valid also for the error codes that carry data in the reference
 *    (wrongCRC / wrongAdler32 / wrongCheck / checksumMismatch).
 *  - *in_consumed reports how far the reference's shared reader would have advanced, so callers can
 *    keep parsing trailers exactly like GzipArchive.swift:88-94 / ZlibArchive.swift:31-37 /
 *    ZipContainer.swift:73-86 / XZBlock.swift:78-82 do.
 *  - thread-safe; never aborts the process.
 */
#ifndef SWC_HIP_H
#define SWC_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "swc_status.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Batched many-buffer launch (the engine proper).  All pointers inside swc_job are DEVICE pointers
 * (HBM-resident input and output); the job array itself is in device memory too.
 * ---------------------------------------------------------------------------------------------- */
typedef enum swc_codec {
    SWC_CODEC_DEFLATE = 1, /* raw RFC 1951 stream      -- Deflate.decompress(_:)   Deflate.swift:30-249; aux: swc_deflate_aux below */
    SWC_CODEC_LZ4_BLOCK = 2, /* one LZ4 block           -- LZ4.process(block:_:)    LZ4.swift:332-413; aux: swc_lz4_aux below */
    SWC_CODEC_LZMA2 = 3,   /* raw LZMA2 chunk stream   -- LZMA2Decoder.decode()    LZMA2Decoder.swift:34-99 */
    SWC_CODEC_LZMA = 4,    /* raw LZMA1 stream         -- LZMADecoder.decode()     LZMADecoder.swift:107-284*/
    SWC_CODEC_BZIP2_BLOCK = 5, /* one bzip2 block body -- BZip2.decode(_:_:)       BZip2.swift:97-270; in / in_len = the stream (any
                              bytes around the block), dict_len = BIT offset of the block body (behind the 48-bit magic and the
                              stored CRC), dict (as an integer) = the stored CRC.  in_consumed is the BIT offset just behind the
                              block.  aux is an OUT field, not read: the bzip2 CRC-32 of out[0 .. out_len) of a block that decoded
                              (SWC_OK, SWC_E_BZIP2_WRONG_CRC), 0 after any other status                                      */
    SWC_CODEC_DELTA = 6,   /* XZ / 7-Zip Delta filter  -- DeltaFilter.decode(_:_:) DeltaFilter.swift:11-33; aux = distance as the
                              reference passes it (XZBlock.swift:57: property + 1), out may equal in            */
    SWC_CODEC_LZ4_COMPRESS = 7, /* ENCODE, one LZ4 block -- LZ4.compress(block:_:) LZ4+Compress.swift:157-281: in = prefix ++ block,
                              dict_len = length of the prefix (dictionary / previous block), out_cap >= n + n / 255 + 16;
                              A valid block for the same bytes, not the reference's bytes            */
    SWC_CODEC_DEFLATE_COMPRESS = 8, /* ENCODE, one raw Deflate stream -- Deflate.compress(data:) Deflate+Compress.swift:22-213: one
                              stored or static-Huffman block over a greedy LZ77 parse; out_cap >= n + n / 8 + 32, out 4-byte
                              aligned; A valid stream for the same bytes, not the reference's bytes.  aux bit 0:
                              the unit is a SEGMENT of a longer stream -- BFINAL clear, an empty stored block behind the block, so
                              that the outputs of consecutive segments, the last one with aux = 0, are one stream           */
    SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC = 9, /* ENCODE, the job contract of 8 (the same parse, out_cap, alignment and aux bit 0); the
                              block is dynamic-Huffman (BTYPE 10, its own code tables, 15-bit codes) where that is strictly
                              smaller than the static block, and stored when not larger than the better of the two (an
                              extension: the reference writes no dynamic block).  Where it is not dynamic, the bytes of 8  */
    SWC_CODEC_LZMA2_COMPRESS = 10 /* ENCODE, one LZMA2 RUN (an extension: the reference has no LZMA encoder): in = the
                              unit, written by one wavefront as chunks of 65,536 bytes -- LZMA (lc 3, lp 0, pb 2, distances up to
                              65,535: dictionary-size byte 8) or stored, whichever is smaller -- behind a dictionary reset, the
                              end marker 0x00 behind the last; out_cap >= n + 3 ceil(n / 65536) + 1, in and out at any alignment.
                              A valid stream for LZMA2Decoder.decode() (LZMA2Decoder.swift:36-74), liblzma and SWC_CODEC_LZMA2.
                              aux bit 0: the unit is a SEGMENT of a longer stream -- no end marker, so that the outputs of
                              consecutive segments, the last one with aux = 0, are one stream.  A CORRECTNESS condition of the
                              bit: the encoder counts positions (pos_state) from the start of its unit, as liblzma does behind
                              a dictionary reset; LZMA2Decoder.decode() and SWC_CODEC_LZMA2 count from the start of the stream.
                              So every segment with a successor must be a multiple of 4 bytes long -- behind one that is not,
                              the joined stream decodes under liblzma only, unless every later chunk up to the next multiple
                              of 4 happens to be stored.  Multiples of 16 make the segments the units that SWC_LZMA2_OPEN
                              and swc_index_blocks kind 8 cut again  */
} swc_codec;

/* aux of an SWC_CODEC_LZ4_BLOCK job (0: an independent block, as ever).  With either bit the launch needs the workspace
 * (SWC_E_NEED_WORKSPACE without one).
 *   SWC_LZ4_LINKED (valid on job i > 0): the job CONTINUES job i - 1 of the array, as the dependent blocks of a frame do
 *     (LZ4.swift:306-313).  A run of linked jobs behind an unlinked HEAD is a chain.  The engine sets
 *     out = jobs[i-1].out + (the bytes of job i - 1 that exist: min(out_len, out_cap)) -- `out` is an OUT field of a linked job,
 *     written back with the result -- and the job's history is the last min(65,536, bytes the chain has produced so far) bytes
 *     in front of `out`, in place; while the chain has produced nothing, the head's adjacent prefix (below) is the history, and
 *     not at all afterwards -- the reference's rule (`out.isEmpty`, LZ4.swift:307-312).
 *     out_cap of every job stays the bound on its OWN output (for a frame: the maximum block size), so the head's buffer must
 *     hold the SUM of the chain's out_cap.  dict must be NULL (else SWC_E_INVALID_ARGUMENT).  The head must be a job of the
 *     two-phase path: linked jobs behind a head whose prefix is NOT adjacent (the lane kernel's job), and linked jobs with no
 *     head in front of them (job 0 and what is linked to it), all report SWC_E_INVALID_ARGUMENT with out_len = in_consumed = 0;
 *     that head itself is decoded as ever.  All blocks of all chains are parsed
 *     in one launch; one wave then carries a chain's blocks through the copy in order.
 *     A failed job of a chain keeps its own status, out_len and in_consumed (a match that reaches in front of the chain's
 *     history: SWC_E_DATA_CORRUPTED with out_len = in_consumed = 0); every job behind it in the chain reports the same status
 *     with out_len = in_consumed = 0.  The first error in order is the one the reference throws.
 *   SWC_LZ4_STORED: `in` is not compressed: it is copied to `out`, out_len = in_consumed = in_len (SWC_E_CAPACITY, nothing
 *     copied, where in_len > out_cap).  For the stored blocks of a chain, whose place nobody knows before the launch.
 * A prefix that is ADJACENT (dict + dict_len == out), on a head or any unlinked job, is history in place as well: with the
 * workspace the job takes the two-phase path (parse, wave copy) like a block without a prefix.  A prefix anywhere else is
 * decoded by the one-block-per-lane kernel, as before. */
typedef enum swc_lz4_aux {
    SWC_LZ4_LINKED = 1,
    SWC_LZ4_STORED = 2
} swc_lz4_aux;

/* aux of an SWC_CODEC_DEFLATE job (0: one whole stream, as ever): the UNITS of a stream that was cut at its flush points.  An
 * empty stored block ends with 00 00 FF FF on a byte boundary and the next block starts on the next byte, so the bytes between
 * two such markers decode on their own -- as long as they refer to nothing in front of themselves (Z_FULL_FLUSH, pigz -i, this
 * library's own segmented encoder).
 *   SWC_DEFLATE_OPEN: the unit may end without a final block.  When the block loop (Deflate.swift:33-44) is about to read a block
 *     header and the reader stands exactly at bit 8 * in_len, the job ends with SWC_OK and in_consumed = in_len.  At any other
 *     position the job behaves like any other (fewer than three bits left: SWC_E_REF_TRAP).  aux is an OUT field too, as for
 *     bzip2: the bit stays set where the unit ended open and is cleared otherwise -- a unit that met a final block ends there
 *     like any stream.  in_len = 0 keeps its status.
 *   SWC_DEFLATE_JOINED (valid on job i > 0): the engine sets out = jobs[i-1].out + min(out_len, out_cap) of job i - 1 -- `out` is
 *     an OUT field, as with SWC_LZ4_LINKED.  A head and the joined jobs behind it are a RUN; the head's buffer must hold the SUM
 *     of the run's out_cap, every out_cap still bounds its job's own output and workspace.  No history is shared: a distance
 *     that reaches in front of the unit's own first byte is SWC_E_REF_TRAP, as ever; every job keeps its own status; a failed or
 *     over-capacity job still occupies min(out_len, out_cap) bytes, and the jobs behind it are placed and decoded normally.
 *     Joined jobs with no head in front of them -- job 0 and what is joined to it -- report SWC_E_INVALID_ARGUMENT with
 *     out_len = in_consumed = 0.
 *   SWC_DEFLATE_LINKED (valid only together with SWC_DEFLATE_JOINED, on job i > 0): the unit SHARES THE HISTORY of the units in front
 *     of it -- what default pigz and Z_SYNC_FLUSH leave between two markers.  The job is placed exactly as a joined job is.  It
 *     continues the CHAIN of job i - 1; the chain's head is the nearest job in front without the bit (which may itself be joined:
 *     a caller that knows a unit stands alone starts a new chain by leaving the bit off), and nothing in front of the head is
 *     history.  The job's history is the last min(32768, out - head's out) bytes in front of its `out`, in place.  A distance that
 *     reaches in front of that history is SWC_E_REF_TRAP: this status replaces whatever status the parse left (a recorded reach
 *     lies in front of whatever stopped the parse, so it is what the reference meets first), out_len, in_consumed and aux stay
 *     as the parse left them, and no byte of the job is written.  Every job keeps its own status, as joined jobs do -- nothing
 *     propagates down the chain: a failed or over-capacity job still occupies min(out_len, out_cap) bytes and the jobs behind it
 *     are placed and copied against whatever lies there (the history never leaves the run's buffer).  The bit without
 *     SWC_DEFLATE_JOINED reports SWC_E_INVALID_ARGUMENT with out_len = in_consumed = 0, and nothing in front of such a job is
 *     history to the jobs behind it; linked jobs with no head -- job 0 and what is joined to it -- report what joined jobs with no
 *     head report.  SWC_DEFLATE_OPEN combines with the bit freely; aux remains an OUT field for the OPEN bit only.
 * All units of all runs are parsed in one launch -- a linked unit with a full history taken for granted, its furthest reach noted;
 * between the parse and the copy one wavefront per 64 jobs places the joined ones (csrc/deflate_place.h), and the copy kernels write
 * every unit byte-exact at whatever address it got, a chain of linked units by ONE wavefront, in order (csrc/deflate_chain.h). */
typedef enum swc_deflate_aux {
    SWC_DEFLATE_JOINED = 1,
    SWC_DEFLATE_OPEN = 2,
    SWC_DEFLATE_LINKED = 4
} swc_deflate_aux;

/* aux of an SWC_CODEC_LZMA2 job: the dictionary-size byte in bits 0-7 (as ever), and above it the bit of a UNIT of a stream that
 * was cut at a dictionary reset.  A chunk that resets the dictionary, the state and the properties (control >= 0xE0, or a stored
 * chunk with control 1 in front of one that resets state and properties) starts a run of chunks that refers to nothing in front
 * of it; swc_index_blocks kind 8 lists the runs.  A run that is not the last has no end marker:
 *   SWC_LZMA2_OPEN: the unit may end without the end marker.  When the chunk loop (LZMA2Decoder.swift:36) is about to read a
 *     control byte and the reader stands exactly at in_len -- and no byte past the end has been read -- the job ends with SWC_OK
 *     and in_consumed = in_len.  At any other position the job behaves like any other (a chunk cut short: SWC_E_REF_TRAP).  aux is
 *     an OUT field for this bit only, as for SWC_DEFLATE_OPEN: it stays set where the unit ended open and is cleared otherwise -- a
 *     unit that met the end marker ends there like any stream; SWC_E_NEED_WORKSPACE leaves aux as it came, so that the same job
 *     list can be launched again with a workspace.  in_len = 0 keeps its status.  No byte at or behind in + in_len is
 *     read, with or without the bit: a unit lies in place inside its stream, the next run's control byte right behind it.
 * A unit counts its output position from 0, and the literal coder and pos_state take their low bits from the position
 * (LZMADecoder.swift:118,136): kind 8 cuts only where the announced sizes in front sum to a multiple of 16, which covers
 * pb, lp <= 4.  A match that reaches in front of the unit fails in the unit (the whole stream may allow it): a caller accepts the
 * units of a stream only if every unit but the last is SWC_OK, still OPEN, in_consumed == in_len and out_len == uncomp_len, and the
 * last is SWC_OK; anything else, and the stream is decoded whole. */
typedef enum swc_lzma2_aux {
    SWC_LZMA2_OPEN = 0x100
} swc_lzma2_aux;

typedef struct swc_job {
    const uint8_t* in;    /* device pointer to the unit's compressed bytes                           */
    uint64_t in_len;
    uint8_t* out;         /* device pointer, caller allocated (OUT for an SWC_LZ4_LINKED / SWC_DEFLATE_JOINED job: set by the engine) */
    uint64_t out_cap;
    uint64_t out_len;     /* OUT: bytes produced; for SWC_E_CAPACITY on Deflate/LZ4: bytes required   */
    uint64_t in_consumed; /* OUT                                                                     */
    int32_t status;       /* OUT: swc_status                                                         */
    int32_t aux;          /* IN : LZMA2 dictionary-size byte, swc_lzma2_aux above it (OUT as well) | LZMA props (lc | lp<<8 | pb<<16) | LZ4: swc_lz4_aux bits | Deflate: swc_deflate_aux bits (OUT as well) | BZIP2: OUT only, the CRC-32 of the block's output (swc_codec above) */
    const uint8_t* dict;  /* IN : LZ4 prefix dictionary (device) or NULL                             */
    uint64_t dict_len;    /* IN : LZ4 dictionary length | BZIP2: bit offset of the block body | LZMA: uncompressed size (UINT64_MAX = unknown) | LZMA dict size in the high half, see swc_hip.h notes */
} swc_job;

typedef struct swc_batch_opts {
    int32_t device;        /* HIP device ordinal, -1 = current                                       */
    void* stream;          /* hipStream_t, NULL = default stream                                     */
    int32_t synchronize;   /* non-zero: wait for completion before returning                         */
    int32_t reserved;
} swc_batch_opts;

/* One launch for all n jobs.  `jobs` is a device pointer to n swc_job records.  Deflate needs an HBM workspace:
 * this entry point allocates it from the stream-ordered pool; swc_batch_decompress_ws takes it from the caller
 * (required for BZip2, recommended for LZ4). */
int swc_batch_decompress(int codec, swc_job* jobs, size_t n, const swc_batch_opts* opts);

/* Scratch bytes the codec needs in HBM (Deflate / LZ4: match records + literal stream of the two-phase path,
 * LZMA: the home of the literal coders (LDS caches four lines of them) and of the long-length trees -- 32 streams per CU and any lc + lp; without it the model
 * of lc + lp <= 4 sits in LDS whole, 5 streams per CU, larger models are refused with SWC_E_NEED_WORKSPACE; BZip2: tt[]).
 * LZ4 also runs without it (one block per lane, much slower on large blocks).  Allocated internally by the single-shot
 * calls; batch callers pass it via swc_batch_decompress_ws. */
size_t swc_batch_workspace_bytes(int codec, size_t n_jobs, uint64_t max_out_cap);
int swc_batch_decompress_ws(int codec, swc_job* jobs, size_t n, void* workspace, size_t workspace_bytes,
                            const swc_batch_opts* opts);

/* CRC-32 (CheckSums.crc32, reference Sources/Common/CheckSums.swift:12-28, as checked by GzipArchive.swift:99)
 * of every job's output, computed on the device after a batch has been decoded: crcs[i] covers
 * out[0 .. min(out_len, out_cap)).  `jobs` and `crcs` are device pointers. */
int swc_batch_crc32(const swc_job* jobs, size_t n, uint32_t* crcs, const swc_batch_opts* opts);

/* swc_batch_decompress_ws and swc_batch_crc32 in one call: decodes the n jobs and leaves in crcs[i] (a device pointer to n
 * words) what swc_batch_crc32 would compute afterwards, for every job whatever its status.  Deflate batches that take the
 * wave copy kernel get the CRC-32 from that kernel: a wave that has written the last byte of its stream folds the stream
 * it has just written, and no separate pass over the outputs runs.  Every other codec (and the small Deflate launches that take
 * the workgroup kernel) decodes and then runs the CRC kernels. */
int swc_batch_decompress_crc32_ws(int codec, swc_job* jobs, size_t n, void* workspace, size_t workspace_bytes, uint32_t* crcs,
                                  const swc_batch_opts* opts);

/* The other checksums of the archive layer over every job's output (same coverage rule), zero-extended to 64 bits:
 *   SWC_SUM_CRC32        CheckSums.crc32       CheckSums.swift:12-28  (GzipArchive.swift:99, XZArchive.swift:109-120)
 *   SWC_SUM_ADLER32      CheckSums.adler32     CheckSums.swift:48-57  (ZlibArchive.swift:38)
 *   SWC_SUM_CRC64        CheckSums.crc64       CheckSums.swift:39-46  (XZArchive.swift:109-120)
 *   SWC_SUM_BZIP2_CRC32  CheckSums.bzip2crc32  CheckSums.swift:30-37  (BZip2.swift:81)
 *   SWC_SUM_XXH32        XxHash32.hash(seed 0) XxHash32.swift:24-83   (LZ4.swift:300,326)
 *   (SHA-256             Sha256.hash           Sha256.swift:28-142    (XZArchive.swift:106-121): 32 bytes, swc_batch_sha256 below)
 * `jobs` and `sums` are device pointers. */
typedef enum swc_checksum {
    SWC_SUM_CRC32 = 1,
    SWC_SUM_ADLER32 = 2,
    SWC_SUM_CRC64 = 3,
    SWC_SUM_BZIP2_CRC32 = 4,
    SWC_SUM_XXH32 = 5
} swc_checksum;
int swc_batch_checksum(int kind, const swc_job* jobs, size_t n, uint64_t* sums, const swc_batch_opts* opts);

/* SHA-256 (Sha256.hash(data:), reference Sources/Common/Sha256.swift:28-142, the block check of an .xz file of check type 0x0A as
 * XZArchive.swift:106-121 verifies it) of every job's output, same coverage rule: digests[32 i .. 32 i + 32) is the digest of
 * out[0 .. min(out_len, out_cap)) of job i, whatever its status, in the standard's byte order.  `jobs` and `digests` are device
 * pointers, `digests` holds 32 * n bytes at any alignment.  A message is hashed by ONE lane (its blocks are one dependent chain):
 * the throughput of a call is the number of its jobs, and a call lasts as long as its longest job.  (The sums of
 * swc_batch_checksum are 64-bit: kind 6 stays SWC_E_INVALID_ARGUMENT there.) */
int swc_batch_sha256(const swc_job* jobs, size_t n, uint8_t* digests, const swc_batch_opts* opts);

/* ------------------------------------------------------------------------------------------------
 * Single-shot calls (host buffers in, malloc()ed host buffer out).
 * ---------------------------------------------------------------------------------------------- */
/* Deflate.decompress(data:) Deflate.swift:24-28 and decompress(_ bitReader:) :30-249
 * (callers GzipArchive.swift:88, ZlibArchive.swift:31, ZipContainer.swift:74) */
int swc_deflate_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t* in_consumed);

/* BZip2.decompress(data:) BZip2.swift:22-26 and decompress(_ bitReader:) :50-95 (caller ZipContainer.swift:82);
 * one stream; *out valid on SWC_E_BZIP2_WRONG_CRC */
int swc_bzip2_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t* in_consumed);
/* BZip2.multiDecompress(data:) BZip2.swift:40-48; sizes[] (swc_free) splits *out per stream */
int swc_bzip2_multi_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t** sizes, size_t* n_streams);

/* LZMA.decompress(data:properties:uncompressedSize:) LZMA.swift:56-73 (caller ZipContainer.swift:89);
 * uncompressed_size < 0 = unknown (end marker required) */
int swc_lzma_decompress(const uint8_t* in, size_t in_len, int lc, int lp, int pb, int64_t dict_size,
                        int64_t uncompressed_size, uint8_t** out, size_t* out_len, size_t* in_consumed);
/* LZMA.decompress(data:) LZMA.swift:25-34 (13-byte .lzma header) */
int swc_lzma_alone_decompress(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len);
/* LZMA2.decompress(_:_:) LZMA2.swift:32-36 (callers XZBlock.swift:51, 7zFolder.swift:159) */
int swc_lzma2_decompress(const uint8_t* in, size_t in_len, uint8_t dict_byte, uint8_t** out, size_t* out_len, size_t* in_consumed);
/* LZMA2.decompress(data:) LZMA2.swift:25-30 (first byte = dictionary size) */
int swc_lzma2_decompress_data(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len);
/* LZMA2.compress(data:) -- an extension, the reference writes no LZMA2: the dictionary-size byte (8) followed by the stream, which
 * is what swc_lzma2_decompress_data takes.  Compressed on the device (SWC_CODEC_LZMA2_COMPRESS; one wavefront per buffer of up to
 * 1 MiB; a larger one is cut into segments of 256 KiB that are compressed in one launch and come out as runs behind dictionary
 * resets -- one LZMA2 stream, which "lzma2_run_bytes" decodes as parallel units).  Empty input: 08 00. */
int swc_lzma2_compress(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);

/* LZ4.decompress(data:dictionary:dictionaryID:) LZ4.swift:73-91; dict NULL = no dictionary,
 * dict_id < 0 = no id passed; *out valid on SWC_E_DATA_CHECKSUM_MISMATCH */
int swc_lz4_decompress(const uint8_t* in, size_t in_len, const uint8_t* dict, size_t dict_len, int64_t dict_id,
                       uint8_t** out, size_t* out_len, size_t* in_consumed);
/* LZ4.compress(data:independentBlocks:blockChecksums:contentChecksum:contentSize:blockSize:dictionary:dictionaryID:)
 * LZ4+Compress.swift:47-155 (LZ4.compress(data:) = independent 1, block checksums 0, content checksum 1, content size 0,
 * 4 MiB blocks, no dictionary).  Frame layout and fields as the reference writes them; the blocks are compressed on the
 * device, all of them in one launch when they are independent (SWC_CODEC_LZ4_COMPRESS).  dict NULL = none, dict_id < 0 =
 * none.  block_size 1..4194304 (the reference's precondition), else SWC_E_INVALID_ARGUMENT. */
int swc_lz4_compress(const uint8_t* data, size_t len, int independent_blocks, int block_checksums, int content_checksum,
                     int content_size, size_t block_size, const uint8_t* dict, size_t dict_len, int64_t dict_id,
                     uint8_t** out, size_t* out_len);
/* Deflate.compress(data:) Deflate+Compress.swift:22-46: one stored or static-Huffman block, compressed on the device
 * (SWC_CODEC_DEFLATE_COMPRESS; one wavefront per buffer of up to 1 MiB; a larger one is cut into segments of 256 KiB that
 * are compressed in one launch and come out as non-final static blocks joined by empty stored blocks -- one Deflate stream).  ZlibArchive.archive(data:) ZlibArchive.swift:54-70: 0x78 0xDA, that stream, Adler-32 of the
 * input (big endian; computed on the host). */
int swc_deflate_compress(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);
int swc_zlib_archive(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);
/* The same with dynamic-Huffman blocks where they are smaller (SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC: every unit and every
 * segment is one block with its own code tables; never larger than the static form, its bytes where no block is dynamic).
 * Parameters as swc_deflate_compress / swc_zlib_archive. */
int swc_deflate_compress_dynamic(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);
int swc_zlib_archive_dynamic(const uint8_t* data, size_t len, uint8_t** out, size_t* out_len);
/* GzipArchive.archive(data:comment:fileName:writeHeaderCRC:isTextFile:osType:modificationTime:extraFields:)
 * GzipArchive.swift:126-240: the header as the reference writes it (magic, CM 8, flags, MTIME, XFL 2, OS, FEXTRA, FNAME,
 * FCOMMENT, FHCRC), Deflate.compress(data) on the device, CRC-32 and ISIZE.  comment / file_name: ISO Latin-1 bytes (NULL =
 * none; the terminating zero is added unless the last byte is one, :134-136 / :147-149 -- the String conversion and its
 * cannotEncodeISOLatin1 are the shim's); os_type: the header byte (FileSystemType+Gzip.swift:23-36, 255 = unknown);
 * has_mtime 0 = four zero bytes, else the low four bytes of `mtime` seconds (:172-178).  Extra fields that sum up (4 + length
 * each) to more than 65,535 bytes: SWC_E_GZIP_CANNOT_ENCODE_ISO_LATIN1, as the reference throws (:190-191). */
typedef struct swc_gzip_extra_field {
    uint8_t si1, si2;
    const uint8_t* bytes;
    size_t len;
} swc_gzip_extra_field;
int swc_gzip_archive(const uint8_t* data, size_t len, const uint8_t* comment, size_t comment_len, const uint8_t* file_name,
                     size_t file_name_len, int write_header_crc, int is_text_file, int os_type, int has_mtime, int64_t mtime,
                     const swc_gzip_extra_field* extra, size_t n_extra, uint8_t** out, size_t* out_len);
/* The same with the body from swc_deflate_compress_dynamic.  Parameters as swc_gzip_archive. */
int swc_gzip_archive_dynamic(const uint8_t* data, size_t len, const uint8_t* comment, size_t comment_len, const uint8_t* file_name,
                             size_t file_name_len, int write_header_crc, int is_text_file, int os_type, int has_mtime, int64_t mtime,
                             const swc_gzip_extra_field* extra, size_t n_extra, uint8_t** out, size_t* out_len);
/* BGZF writer (an extension: the reference writes no BGZF; SAM/BAM specification 4.1).  The input is cut into chunks of
 * block_size bytes (1..65280; 0 = 65280 = 0xFF00, what bgzip cuts; more: SWC_E_INVALID_ARGUMENT), every chunk becomes one gzip
 * member -- 1f 8b 08 04, MTIME 0, XFL 0, OS 255, the extra field 'BC' with BSIZE = member size - 1, ONE final Deflate block as
 * SWC_CODEC_DEFLATE_COMPRESS (dynamic != 0: SWC_CODEC_DEFLATE_COMPRESS_DYNAMIC) writes it, CRC-32 and ISIZE of the chunk -- and
 * the 28-byte end-of-file member closes the file, for empty input too.  All members are compressed in one launch, summed, and packed
 * one behind the other on the device (csrc/bgzf_pack.h).  The result decodes in one launch through swc_gzip_multi_unarchive /
 * swc_index_blocks kind 1.
 *   swc_bgzf_bound            the largest file `len` bytes can become: len + 31 * ceil(len / block_size) + 28 (0: bad block_size)
 *   swc_bgzf_workspace_bytes  device scratch of swc_batch_bgzf_archive for that input (job lists, offsets, a slot per member)
 *   swc_batch_bgzf_archive    device-resident: src, dst, total (one uint64), member_sizes (n + 1 uint64 -- the size of every member,
 *                             the end-of-file member last -- or NULL) and workspace are DEVICE pointers.  Returns when its kernels
 *                             have run (the status is the outcome of the device work, whatever opts->synchronize says): the first
 *                             compress error by member index, SWC_E_CAPACITY with the needed length in *total and no byte written
 *                             when the file does not fit dst_cap, SWC_E_NEED_WORKSPACE when the workspace is too small.
 *   swc_bgzf_archive          host buffers; *sizes (swc_free, `sizes` may be NULL) = the size of every member incl. the end-of-file
 *                             member.  The input is staged once and packed in rounds of 16,384 members (1 GiB), so the device
 *                             scratch stays near 1.2 GB whatever the input; every round lands at its place in the result. */
size_t swc_bgzf_bound(size_t len, size_t block_size);
size_t swc_bgzf_workspace_bytes(size_t len, size_t block_size);
int swc_batch_bgzf_archive(const uint8_t* src, uint64_t len, uint64_t block_size, int dynamic, uint8_t* dst, uint64_t dst_cap,
                           uint64_t* total, uint64_t* member_sizes, void* workspace, size_t workspace_bytes, const swc_batch_opts* opts);
int swc_bgzf_archive(const uint8_t* data, size_t len, size_t block_size, int dynamic, uint8_t** out, size_t* out_len, size_t** sizes,
                     size_t* n_members);
/* BZip2.compress(data:blockSize:) BZip2+Compress.swift:40-74 (BZip2.compress(data:) :19-21 = block_size 1).  block_size 1..9 =
 * BlockSize.one ... .nine (else SWC_E_INVALID_ARGUMENT); the input is cut into blocks of block_size x 80,000 bytes as the
 * reference cuts it (:46), all blocks are compressed on the device together: initial run-length coding, Burrows-Wheeler
 * transform (prefix doubling over all blocks at once), move-to-front and zero-run coding, Huffman coding with up to six
 * tables per block, one per group of 50 symbols, refined in four passes over all groups (bzip2's scheme).  The stream decodes
 * to `data` with the reference's decoder and with libbz2; its bytes are not the reference encoder's (which builds each of its
 * tables from a single group of 50 symbols). */
int swc_bzip2_compress(const uint8_t* data, size_t len, int block_size, uint8_t** out, size_t* out_len);
/* LZ4.multiDecompress(data:dictionary:dictionaryID:) LZ4.swift:116-146 */
int swc_lz4_multi_decompress(const uint8_t* in, size_t in_len, const uint8_t* dict, size_t dict_len, int64_t dict_id,
                             uint8_t** out, size_t* out_len, size_t** sizes, size_t* n_frames);

/* Host-side framing around the batch API (reference L3 "archives") */
/* GzipArchive.unarchive(archive:) GzipArchive.swift:38-48 */
int swc_gzip_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len);
/* GzipArchive.multiUnarchive(archive:) GzipArchive.swift:62-77; sizes[] splits *out per member.  A BGZF file decodes in one launch; a
 * file of plain members member by member, or -- swc_set_tuning "gzip_member_scan" = 1 -- from one launch over its candidate members */
int swc_gzip_multi_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t** sizes, size_t* n_members);
/* ZlibArchive.unarchive(archive:) ZlibArchive.swift:25-42 */
int swc_zlib_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len);
/* XZArchive.unarchive(archive:) XZArchive.swift:27-51 / splitUnarchive :69-88 */
int swc_xz_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len);
int swc_xz_split_unarchive(const uint8_t* in, size_t in_len, uint8_t** out, size_t* out_len, size_t** sizes, size_t* n_streams);
/* XZArchive.archive(data:) -- an extension, the reference writes no .xz: ONE stream -- the stream header, one block per block_size
 * bytes of data (0: 262,144; else a multiple of 16 in 4,096 .. 2^30), the index, the footer.  A block's header carries flags 0xC0,
 * both size fields and the LZMA2 filter with dictionary-size byte 8 (the layout of a multi-threaded xz, which readers split by);
 * its data are one SWC_CODEC_LZMA2_COMPRESS run.  All blocks are compressed in ONE launch; their checks (check_type 0 none,
 * 1 CRC-32, 4 CRC-64, 10 SHA-256; anything else SWC_E_INVALID_ARGUMENT) are taken on the device over the staged data (SHA-256: from
 * "sha256_device_min_units" blocks on, below that by swc_sha256); the CRC-32s of the headers, the index and the footer on the host.
 * Empty data: the 32-byte archive without a block, answered without a device. */
int swc_xz_archive(const uint8_t* data, size_t len, int check_type, size_t block_size, uint8_t** out, size_t* out_len);

/* Many independent archives in one call: host-side block discovery + ONE batched launch.
 * archives[i]/lens[i] are host buffers; outs[i]/out_lens[i]/statuses[i] are filled per archive
 * (outs[i] released with swc_free).  kind: 1 = gzip member (incl. BGZF), 2 = zlib stream,
 * 3 = raw deflate, 4 = LZ4 frame, 5 = bzip2 stream, 6 = xz stream, 7 = raw LZMA2 (first byte = dict byte).
 * An archive that fails in its header -- before the reference would decode any payload -- contributes nothing to the launch, as in
 * the single-shot calls: a set of nothing but such archives is answered without a device; any other set returns SWC_E_DEVICE there. */
int swc_unarchive_many(int kind, const uint8_t* const* archives, const size_t* lens, size_t n,
                       uint8_t** outs, size_t* out_lens, int32_t* statuses);
/* The same over several GPUs of one node (the reference has no counterpart: its callers loop over archives on one core).
 * devices[0..n_devices) are HIP device ordinals (a device may be listed more than once); the archive list is cut into one
 * contiguous range per entry, balanced by compressed + uncompressed bytes (the uncompressed size where the framing declares
 * it -- gzip ISIZE, LZ4 content size -- else the compressed size again), and every range is decoded on its device by that
 * device's worker thread (one per device for the life of the process: its stream and page-locked staging buffers are set up
 * once).  The archives are independent, so there is no exchange between devices; results land at their archive's index
 * exactly as swc_unarchive_many returns them.  SWC_E_DEVICE if an ordinal does not name a gfx950 device (the calling
 * thread's own current device does not matter). */
int swc_unarchive_many_devices(int kind, const uint8_t* const* archives, const size_t* lens, size_t n,
                               const int* devices, size_t n_devices, uint8_t** outs, size_t* out_lens, int32_t* statuses);

/* Block discovery on the host, as a library call (no device needed) -- what swc_unarchive_many / the multi-member entry
 * points use internally, for callers that stage their data on the device themselves:
 *   kind 1  BGZF: every gzip member that carries the 'BC' extra field (GzipHeader.swift:110-156): offset / comp_len of its
 *           Deflate stream, uncomp_len = ISIZE.  SWC_E_INVALID_ARGUMENT if a member lacks the field.
 *   kind 3  raw Deflate: the units the stream can be cut into -- a cut behind every 00 00 FF FF (the end of an empty stored block),
 *           cuts merged until every unit but the last holds at least "deflate_unit_bytes" (swc_set_tuning; 0: one unit), no cut
 *           at the very end of the buffer.  aux = the swc_deflate_aux bits of the unit's job (all but the first JOINED -- and LINKED,
 *           with "deflate_units_linked" = 1 -- all but the last OPEN).  The markers are candidates -- they occur in stored data and in codes: a caller checks the result
 *           as the single-shot calls do (every unit in front of some unit k SWC_OK, still OPEN, in_consumed == in_len; unit k
 *           SWC_OK with the bit cleared) and decodes the stream whole otherwise.
 *   kind 4  LZ4 frame (LZ4.swift:278-299): the blocks of the frame the buffer opens with; aux = 1 for stored blocks; flags
 *           bit 0 = the block continues its predecessor (every block but the first of a frame with dependent blocks: a job
 *           with SWC_LZ4_LINKED), 0 throughout a frame of independent blocks.
 *   kind 5  bzip2: every BIT offset of the 48-bit block magic (BZip2.swift:74-88) -- candidates, a magic may occur in data.
 *   kind 6  xz: the LZMA2-only blocks listed by the index of every stream (XZArchive.swift:132-192 read backwards):
 *           offset / comp_len of the LZMA2 data, uncomp_len, aux = dictionary-size byte.
 *   kind 7  raw LZMA2 (first byte = dictionary-size byte): the chunk walk of LZMA2Decoder.decode() / dispatch()
 *           (LZMA2Decoder.swift:36-74) without the LZMA decode: one ref per chunk, offset of its control byte, comp_len =
 *           header + payload, uncomp_len, aux = control byte, flags bit 0 = the chunk resets the dictionary (a run of
 *           chunks that decodes on its own starts here), bit 1 = it carries a properties byte.  The end marker is not
 *           listed.  Returns SWC_E_LZMA2_WRONG_CONTROL_BYTE (:47-48) or SWC_E_REF_TRAP (a chunk runs past the buffer)
 *           with the chunks before the error in refs / *n.
 *   kind 8  raw LZMA2 (first byte = dictionary-size byte): the UNITS the stream can be cut into at its dictionary resets
 *           (swc_lzma2_aux).  With P = the sum of the unpack sizes the chunks in front of a chunk announce, a chunk is a cut
 *           candidate iff P > 0, P % 16 == 0, and its control byte is >= 0xE0, or is 1 and the first chunk behind it that is not
 *           stored (control >= 0x80), if there is one, has control >= 0xC0.  Candidates are merged until every unit but the last
 *           holds at least "lzma2_run_bytes" compressed bytes (swc_set_tuning; 0: one unit).  offset from `in`; the last
 *           unit runs to the end of the buffer; uncomp_len = the sum of the unit's announced sizes (exact for a unit that
 *           decodes); aux = the dictionary-size byte | SWC_LZMA2_OPEN on all but the last; flags = 0.  A stream the walk cannot
 *           follow (a wrong control byte, a chunk past the end) is ONE unit and SWC_OK: its decode reports the error.  The units
 *           are candidates -- a match may reach behind a reset: a caller checks the result by the rule at swc_lzma2_aux.
 *   kind 9  plain gzip members: every place a member MAY start, without a decode -- THE CANDIDATE RULE, which this kind states on the
 *           host, csrc/gzip_scan.h on the device (swc_batch_gzip_index) and swc_gzip_multi_unarchive relies on ("gzip_member_scan").
 *           Byte offset p of a buffer of len bytes is a candidate iff p + 20 <= len (10 header bytes, the 2-byte empty static block,
 *           8 trailer bytes), in[p] == 0x1f, in[p+1] == 0x8b, in[p+2] == 0x08 and (in[p+3] & 0xE0) == 0 -- the magic, method and
 *           reserved-flag tests of GzipHeader.swift:73-88 and nothing else; candidates may lie 3 bytes apart.  `next` of a candidate
 *           is the offset of the candidate behind it, len for the last.  Its data position is p + 10, + 2 + XLEN with FEXTRA (the
 *           sub-fields are not walked), + the zero-terminated FNAME and FCOMMENT where flagged -- each at most 256 bytes INCLUDING
 *           its zero -- + 2 with FHCRC; every read in front of len.  One ref per candidate, in ascending order of p.  A usable ref
 *           (flags bit 0 clear): offset = the data position, comp_len = next - offset - 8, uncomp_len = the little-endian 32-bit
 *           word at next - 4 (the ISIZE the member has if the next candidate is where it ends), aux = offset - p.  A candidate
 *           whose header leaves the buffer, whose name exceeds the limit (a condition, not a tuning: it bounds what one thread
 *           reads of a hostile buffer; the walk decodes such a member) or whose data position + 10 > next is UNUSABLE: flags bit 0
 *           set, offset = p, comp_len = uncomp_len = aux = 0.  Candidates are guesses -- the pattern occurs in names, in stored
 *           data and in codes: a caller decodes the usable ones and keeps a result only where a sequential walk that starts at
 *           offset 0 arrives at p, gzip_member_prepare puts the data where the ref did, the unit is SWC_OK with in_consumed ==
 *           comp_len and uncomp_len bytes of output, and CRC-32 and ISIZE match (framing_deflate.cpp).
 *   kind 10 bzip2 marks: every place a block or the end of a stream MAY start, without a decode -- THE MARK RULE, which this kind
 *           states on the host, csrc/bzip2_scan.h on the device (swc_batch_bzip2_index) and the bzip2 decoders rely on
 *           ("bzip2_scan_bytes").  Bits are numbered MSB-first, as MsbBitReader reads them: bit k of the buffer is bit 7 - (k & 7) of
 *           byte k >> 3; L = 8 * len.  Bit offset b is a mark iff b >= 32 (behind a stream header), b + 80 <= L, and the 48 bits from
 *           b are 0x314159265359 (a block) or 0x177245385090 (the end of a stream).  The 80 bits are the magic and the 32-bit word
 *           behind it: the walk (BZip2.swift:71) reports wrongMagic wherever fewer than 80 bits are left, before it looks at a block,
 *           so a shorter candidate is never needed and there is no unusable form.  One ref per mark, in ascending order of b:
 *           offset = b (bits, as kind 5), comp_len = next - b in bits, `next` the offset of the mark behind it and L for the last,
 *           uncomp_len = 0, aux = the 32 bits at b + 48, MSB-first (a block's stored CRC, or the stream's combined CRC), flags bit 0
 *           = the end of a stream.  Marks are candidates -- a magic may occur in data: a caller uses one only where a sequential
 *           walk arrives at it, as with kind 5.  The block marks are exactly the kind-5 refs with offset + 80 <= L.
 * *n receives the number found; up to `cap` are written. */
typedef struct swc_block_ref {
    uint64_t offset;      /* bytes from `in` (kinds 5 and 10: bits) */
    uint64_t comp_len;
    uint64_t uncomp_len;  /* 0 = not known from the framing */
    uint32_t aux;
    uint32_t flags;       /* kinds 4, 7, 9 and 10 only, else 0 */
} swc_block_ref;
int swc_index_blocks(int kind, const uint8_t* in, size_t len, swc_block_ref* refs, size_t cap, size_t* n);
/* swc_index_blocks kind 9 for a buffer in HBM (csrc/gzip_scan.h: two passes over the buffer, a ref per candidate; an extension).  src,
 * refs, n and workspace are DEVICE pointers; src and refs at any alignment.  *n receives the number of candidates found -- it may
 * exceed cap; refs[0 .. min(*n, cap)) are written, each as an unlimited call writes it, and nothing behind them.  len == 0: *n = 0.
 * The kernels run on opts->stream, and the call waits for them with opts->synchronize, as swc_batch_checksum does.
 * SWC_E_INVALID_ARGUMENT: a null pointer (src with len != 0, refs with cap != 0, n, workspace); SWC_E_NEED_WORKSPACE: workspace_bytes
 * is less than swc_gzip_index_workspace_bytes(len, cap), nothing is written; SWC_E_DEVICE.
 *   swc_gzip_index_workspace_bytes  device scratch of that call: 12 bytes per 16 KiB of the buffer and 8 per ref that can be written */
size_t swc_gzip_index_workspace_bytes(uint64_t len, uint64_t cap);
int swc_batch_gzip_index(const uint8_t* src, uint64_t len, swc_block_ref* refs, uint64_t cap, uint64_t* n, void* workspace,
                         size_t workspace_bytes, const swc_batch_opts* opts);
/* swc_index_blocks kind 10 for a buffer in HBM (csrc/bzip2_scan.h: one pass over the buffer, a second one over the 16 KiB tiles that
 * hold marks, a ref per mark; an extension).  The contract is that of swc_batch_gzip_index: src, refs, n and workspace are DEVICE
 * pointers; src and refs at any alignment.  *n receives the number of marks found -- it may exceed cap; refs[0 .. min(*n, cap)) are
 * written, each as an unlimited call writes it, and nothing behind them.  len == 0: *n = 0.  The kernels run on opts->stream, and
 * the call waits for them with opts->synchronize.  SWC_E_INVALID_ARGUMENT: a null pointer (src with len != 0, refs with cap != 0, n,
 * workspace); SWC_E_NEED_WORKSPACE: workspace_bytes is less than swc_bzip2_index_workspace_bytes(len, cap), nothing is written;
 * SWC_E_DEVICE.  A ref becomes a SWC_CODEC_BZIP2_BLOCK job over src: dict_len (the bit offset of the block's body) = offset + 80,
 * dict (the stored CRC) = aux.
 *   swc_bzip2_index_workspace_bytes  device scratch of that call: 12 bytes per 16 KiB of the buffer and 8 per ref that can be written */
size_t swc_bzip2_index_workspace_bytes(uint64_t len, uint64_t cap);
int swc_batch_bzip2_index(const uint8_t* src, uint64_t len, swc_block_ref* refs, uint64_t cap, uint64_t* n, void* workspace,
                          size_t workspace_bytes, const swc_batch_opts* opts);

/* ZipContainer.getEntryData (reference Sources/ZIP/ZipContainer.swift:61-118) for all entries of one container: every
 * entry is an independent stream whose location and sizes the caller already has from the central directory
 * (ZipEntryInfoHelper.swift:22-44), so the Deflate (8) and LZMA (14) entries go to the device as ONE batch each; stored (0)
 * entries are copied, BZip2 (12) entries run their own block discovery.  Per entry: status (DeflateError / BZip2Error /
 * LZMAError / SWC_E_ZIP_WRONG_SIZE / SWC_E_ZIP_COMPRESSION_NOT_SUPPORTED), crc_error (the caller raises
 * ZipError.wrongCRC(entries so far), ZipContainer.swift:52-53) and the data (malloc()ed, swc_free). */
typedef struct swc_zip_entry {
    uint64_t data_offset;        /* IN : helper.dataOffset                                             */
    uint64_t comp_size;          /* IN : helper.compSize                                               */
    uint64_t uncomp_size;        /* IN : helper.uncompSize                                             */
    uint32_t crc32;              /* IN : helper.entryInfo.crc                                          */
    uint16_t method;             /* IN : 0 copy, 8 deflate, 12 bzip2, 14 lzma (CompressionMethod+Zip.swift:9-21) */
    uint8_t has_data_descriptor; /* IN : helper.hasDataDescriptor                                      */
    uint8_t zip64;               /* IN : helper.zip64FieldsArePresent                                  */
    int32_t status;              /* OUT                                                                */
    uint8_t crc_error;           /* OUT                                                                */
    uint8_t pad[3];
    uint8_t* data;               /* OUT: entry data (empty on error)                                   */
    size_t data_len;             /* OUT                                                                */
} swc_zip_entry;
int swc_zip_get_entries_data(const uint8_t* container, size_t len, swc_zip_entry* entries, size_t n);

/* SevenZipFolder.unpack(data:) (reference Sources/7-Zip/7zFolder.swift:138-194) for many folders at once.  The caller has
 * parsed the archive header and hands over, per folder, its packed stream and the ORDERED coder chain (orderedCoders(),
 * :88-97) with each coder's unpack size (unpackSize(for:), :129-136).  Folders are independent: stage k of all chains
 * runs as one batched launch per codec.  method: 0 copy, 1 deflate, 2 bzip2, 3 LZMA2, 4 LZMA, 5 Delta (id 03),
 * 6 LZ4 (id 04 F7 11 04), 7 an encryption method, 8 anything else.  Per folder: status (the codec's error,
 * SWC_E_7Z_*), data (malloc()ed, swc_free; empty on error). */
typedef struct swc_7z_coder {
    uint32_t method;
    uint8_t props[5];        /* coder.properties (LZMA2: 1 byte, LZMA: 5, Delta: 1)                          */
    uint8_t props_len;       /* 0xFF = properties absent                                                     */
    uint8_t multi_stream;    /* !(numInStreams == 1 || numOutStreams == 1), 7zFolder.swift:141               */
    uint8_t pad;
    uint64_t unpack_size;
} swc_7z_coder;
typedef struct swc_7z_folder {
    const uint8_t* data;     /* IN : packed stream of the folder                                             */
    size_t len;
    const swc_7z_coder* coders;
    size_t n_coders;
    int32_t status;          /* OUT                                                                          */
    int32_t pad;
    uint8_t* out;            /* OUT                                                                          */
    size_t out_len;
} swc_7z_folder;
int swc_7z_unpack_folders(swc_7z_folder* folders, size_t n);

/* checksums used by the framing layer (CheckSums.swift:12-57, XxHash32.swift:24-83, Sha256.swift:28-142) */
uint32_t swc_crc32(const uint8_t* p, size_t n, uint32_t prev);
uint32_t swc_adler32(const uint8_t* p, size_t n);
/* the sum of A ++ B from the sums of A and B and the length of B (the units of a Deflate run are summed one by one on the device) */
uint32_t swc_crc32_combine(uint32_t a, uint32_t b, size_t len_b);
uint32_t swc_adler32_combine(uint32_t a, uint32_t b, size_t len_b);
uint64_t swc_crc64(const uint8_t* p, size_t n);
uint32_t swc_bzip2_crc32(const uint8_t* p, size_t n);
uint32_t swc_xxh32(const uint8_t* p, size_t n, uint32_t seed);
void swc_sha256(const uint8_t* p, size_t n, uint8_t digest[32]);

void swc_free(void* p);
/* What the library keeps between calls -- freed device memory in the device's pool (4 GiB), the calling thread's two page-locked
 * staging buffers (512 MiB each), large host results handed back through swc_free() (512 MiB in all) -- goes back to the
 * driver / the system: the parked results, the CALLING thread's staging buffers, the current device's pool.  The limits:
 * swc_set_tuning "pool_keep_mib" / "pinned_keep_mib" / "result_cache_mib" (or the environment variables SWC_POOL_KEEP_MIB /
 * SWC_PINNED_KEEP_MIB / SWC_RESULT_CACHE_MIB, read when the library is loaded).  Returns SWC_OK. */
int swc_trim(void);
/* 1 if a gfx950 device is usable, 0 otherwise (then every decode entry point returns SWC_E_DEVICE) */
int swc_device_available(void);
const char* swc_version(void);
/* Knobs that never change results.  Memory kept between calls (see swc_trim): "pool_keep_mib", "pinned_keep_mib",
 * "result_cache_mib" = MiB (>= 0).  Measurement knobs, meant for benchmarking:
 *   "phase_timing" = 0 | 1      HIP events between the kernels of the batch launches of the CALLING THREAD (like the launch
 *                               stream and the staging buffers, measurement state is per thread);
 *   "lzma_coder_cache" = 1 | 0  process-wide: LZMA / LZMA2 launches with a workspace keep four LINES (a third of a literal
 *                               coder each) in LDS as a cache of the coders in the workspace (32 streams per CU, default) or
 *                               all coders of lc + lp <= 3 in LDS (10 streams per CU);
 *   "lz_copier" = 1 | 0 | -1    process-wide: the LZ77 copy phase of Deflate / LZ4 launches -- 1 (default): one stream
 *                               per wave (csrc/lz_copy.h: Deflate a 6 KiB LDS window in groups of up to 1 KiB, LZ4 7 KiB / 1 KiB)
 *                               for launches of 2,560 streams and more, one stream per 512-thread workgroup
 *                               (csrc/lz_resolve.h) below; 0: the workgroup kernel always; -1: the wave kernel whatever the
 *                               launch size;
 *   "deflate_team" = 1 | 0 | -1 process-wide: Deflate launches of up to 256 streams give every stream a workgroup of six wavefronts
 *                               (csrc/inflate_sync.h: the master on the job, the helpers on the rounds behind the master's --
 *                               the latency of ONE stream is a wave's, and a team cuts it by three) (1, default), one wavefront
 *                               per stream whatever the launch (0), or a team up to 4,096 streams (-1: tests);
 *   "bzip2_hot_cxx" = 0 | 1     process-wide: BZip2 launches run the instantiation of the block kernel whose plain-symbol loop is
 *                               compiled from C++ (1) instead of the hand-written assembly (0, default) -- the two are compared
 *                               by the GPU tests;
 *   "bzip2_team_walk" = 1 | 0 | 2   process-wide: BZip2 launches run stage 3 -- the inverse Burrows-Wheeler walk, the lay-out,
 *                               the RLE1 undo -- as kernels of their own that walk out of the XCDs' L2 (csrc/bzip2_team.h)
 *                               unless the launch is tiny (1, default), never (0: one wavefront takes a block through all
 *                               stages), or always (2);
 *   "deflate_unit_bytes" = n >= 0   process-wide: the Deflate decoders (swc_deflate_decompress, swc_gzip_unarchive,
 *                               swc_gzip_multi_unarchive, swc_zlib_unarchive, swc_unarchive_many kinds 1-3) cut a stream behind the
 *                               empty stored blocks it holds into units of at least n compressed bytes that decode in parallel in
 *                               one launch (32768 is the value the tests and tools/exp_deflate_units.py use); a stream whose units do not stand alone is decoded whole afterwards
 *                               (swc_stat "deflate_unit_fallbacks"); 0 (default, until the gain is measured: DESIGN.md 4.1.1): never cut;
 *   "deflate_units_linked" = 0 | 1   process-wide: the units "deflate_unit_bytes" cuts -- and swc_index_blocks kind 3 lists -- are
 *                               SWC_DEFLATE_LINKED as well, all but the first: they share the history of the units in front of them, so
 *                               streams whose units reach back (default pigz, Z_SYNC_FLUSH) decode as units instead of falling back;
 *                               0 (default): units that stand alone, as before;
 *   "gzip_member_scan" = 0 | 1  process-wide: swc_gzip_multi_unarchive, for a file that is not BGZF, stages the file once, finds every
 *                               place a member may start on the device (swc_index_blocks kind 9, csrc/gzip_scan.h), decodes the plausible
 *                               candidates ahead in ONE launch and lets its sequential walk take from that launch every member that is
 *                               exactly what the walk's own decode would have been accepted as (swc_stat "gzip_scan_members"); the walk
 *                               decodes whatever else it meets itself (swc_stat "gzip_scan_walked"), so results, errors and partial
 *                               results are the same.  A file with fewer than two candidates, or more than max(4096, len / 256), is
 *                               walked as before.  0 (default): never -- it ships as 0; flipping it is a follow-up that cites
 *                               profiles/gzip_members.txt;
 *   "bzip2_scan_bytes" = n >= 0   process-wide: the bzip2 decoders (swc_bzip2_decompress, swc_bzip2_multi_decompress,
 *                               swc_unarchive_many / swc_unarchive_many_devices kind 5, the BZip2 entries of swc_zip_get_entries_data)
 *                               stage an archive of at least n bytes once and find its marks on the device (swc_index_blocks kind 10,
 *                               csrc/bzip2_scan.h) instead of scanning it on the host; every ref is checked against the host copy
 *                               before it is used, the blocks are decoded from the staged copy, and the unchanged sequential walk
 *                               decides, so results, errors and partial results are the same (swc_stat "bzip2_scan_files",
 *                               "bzip2_scan_marks").  Room for max(4096, len / 4096) marks; a file with more is indexed once more with
 *                               room for all.  Any device failure: the host scans.  0 (default): never -- it ships as 0; flipping
 *                               it is a follow-up that cites profiles/bzip2_scan.txt;
 *   "lzma2_run_bytes" = n >= 0   process-wide: the LZMA2 decoders (swc_lzma2_decompress, swc_lzma2_decompress_data, the blocks of
 *                               swc_xz_unarchive / swc_xz_split_unarchive, swc_unarchive_many kinds 6 and 7, method 3 of
 *                               swc_7z_unpack_folders) cut a stream at its dictionary resets (swc_index_blocks kind 8) into units
 *                               of at least n compressed bytes that decode in parallel in one launch (swc_stat "lzma2_run_units");
 *                               a stream whose units do not stand alone -- a match that reaches behind a reset, any error -- is
 *                               decoded whole afterwards and that result is reported (swc_stat "lzma2_run_fallbacks");
 *                               0 (default): never cut -- it ships as 0; flipping it is a follow-up that cites
 *                               profiles/lzma2_runs.txt;
 *   "sha256_device_min_units" = n >= 1   process-wide: the SHA-256 checks of .xz blocks (swc_xz_unarchive, swc_xz_split_unarchive,
 *                               swc_unarchive_many kind 6) are computed on the device, behind the decode, when the launch that decodes the
 *                               blocks ahead holds at least n of them; below, by swc_sha256 on the host as the walk reaches them
 *                               (default 32, measured: DESIGN.md 4.3.1);
 *   "bgzf_round_members" = 1..16384   process-wide, for tests: members per round of swc_bgzf_archive (default 16384); the file is
 *                               the same bytes whatever the round size. */
int swc_set_tuning(const char* key, int value);
/* Profile builds of the library (-DSWC_PROFILE) only: a device buffer of 32 x uint64 per job of the next Deflate
 * launches that the kernels fill with cycle counts per stage (tools/exp_profile.py).  NULL switches it off.  A no-op in
 * the shipped build. */
int swc_set_profile_buffer(void* device_ptr);
/* With "phase_timing" on: durations (ms) of the kernels of the calling thread's last batch launch, in launch order --
 * Deflate: entropy decode, LZ77 resolve; LZ4: dictionary-block kernel, parse, resolve; BZip2: block kernel (Huffman + MTF,
 * counting sort, walk), with "bzip2_team_walk" the team walk and the team finish, serial fallback, block CRC; LZMA / LZMA2:
 * the one kernel; swc_batch_bgzf_archive: compress, CRC-32 of the chunks, offsets + pack.  Returns the number of values written (0 if none or if `cap` is too small; at most 5). */
int swc_last_phase_ms(float* ms, int cap);

/* Process-wide launch statistics of the host framing layer (monotonic, for tests and tuning): "launches" = batched
 * launches issued by the single-shot / many-archive entry points, "units" = units decoded by them, "xz_cache_hits" =
 * .xz blocks the sequential walk took from the index-driven ahead-of-time batch, "deflate_unit_fallbacks" = Deflate streams that
 * were cut into units and had to be decoded whole after all, "sha256_device_units" = .xz blocks whose SHA-256 check the walk
 * took from the device, "lzma2_run_units" = the units of the LZMA2 streams that were cut at their dictionary resets and
 * accepted, "lzma2_run_fallbacks" = LZMA2 streams that were cut and had to be decoded whole after all, "gzip_scan_members" = members
 * of plain multi-member gzip files that the walk took from the launch ahead ("gzip_member_scan"), "gzip_scan_walked" = members of
 * such scanned files that the walk had to decode itself, "bzip2_scan_files" = bzip2 archives whose marks the device found
 * ("bzip2_scan_bytes"), "bzip2_scan_marks" = the block marks taken from it.  Unknown key: -1. */
long long swc_stat(const char* key);

#ifdef __cplusplus
}
#endif
#endif /* SWC_HIP_H */
