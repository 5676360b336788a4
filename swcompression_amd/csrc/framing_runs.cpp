// framing_runs.cpp -- streams through the engine as runs of units: the host protocol shared by the codecs whose streams can be cut
// (RunCodec in framing.h: Deflate at flush points, LZMA2 at dictionary resets), and the one-unit forms of a launch.
//
// A cut is only a guess -- the bytes of a marker occur in data too, a unit may reach behind its start -- and the guess is checked by
// the decode itself: the result of the units stands only if every unit in front of the one that met the end of the stream ended
// open exactly at its last byte with SWC_OK, and that one is SWC_OK; by induction that is what the sequential parse does.  Anything
// else -- a false cut, a unit that reaches back where it may not, any error -- and the stream is decoded whole, as ever, and THAT
// result is reported: error order, error-carried data and the quirks stay exact.
#include <vector>
#include "framing.h"

namespace swc {

HostUnit unit_of(const HostUnit& st, const BlockRef64& ref) {
    HostUnit u;
    u.in = st.in + ref.offset;
    u.in_len = (size_t)ref.comp_len;
    u.base = st.base ? st.base : st.in;
    u.base_len = st.base ? st.base_len : st.in_len;
    u.aux = (int32_t)ref.aux;
    return u;
}

static int run_cut(const RunCodec& c, std::vector<HostUnit>& streams) {
    const size_t least = c.least_bytes();
    struct Run { size_t stream, first; };
    std::vector<Run> runs;
    std::vector<std::vector<BlockRef64>> refs(streams.size());   // empty: the stream stays whole
    if (least != 0)
        for (size_t s = 0; s < streams.size(); s++) {
            const HostUnit& u = streams[s];
            if (u.in_len > least && !u.dict && !u.chain) c.index(u, least, refs[s]);
            if (refs[s].size() >= 2) runs.push_back({s, 0});
            else refs[s].clear();
        }
    if (runs.empty()) return run_units(c.codec, streams);
    // one list for one launch, in the streams' order: the streams that stay whole as they are, every other one as its run, head first
    std::vector<HostUnit> units;
    std::vector<size_t> whole_at(streams.size(), (size_t)-1);
    std::vector<std::vector<uint8_t>> joined(runs.size());
    auto add_run = [&](std::vector<HostUnit>& list, size_t r, const HostUnit* again) {
        const size_t s = runs[r].stream, first = list.size();
        for (const BlockRef64& f : refs[s]) list.push_back(unit_of(streams[s], f));
        c.fill(streams[s], refs[s], &list[first], again, joined[r]);
        return first;
    };
    for (size_t s = 0, r = 0; s < streams.size(); s++) {
        if (refs[s].empty()) { whole_at[s] = units.size(); units.push_back(std::move(streams[s])); }
        else { runs[r].first = add_run(units, r, nullptr); r++; }
    }
    int rc = run_units(c.codec, units);
    if (rc != SWC_OK) return rc;
    if (c.once_more) {   // all the runs that ask for it, together
        std::vector<HostUnit> again;
        std::vector<size_t> which;
        for (size_t r = 0; r < runs.size(); r++)
            if (c.once_more(&units[runs[r].first])) { which.push_back(r); add_run(again, r, &units[runs[r].first]); }
        if (!again.empty()) {
            rc = run_units(c.codec, again);
            if (rc != SWC_OK) return rc;
            size_t at = 0;
            for (size_t r : which)
                for (size_t k = 0; k < refs[runs[r].stream].size(); k++) units[runs[r].first + k] = std::move(again[at++]);
        }
    }
    for (size_t s = 0; s < streams.size(); s++) if (whole_at[s] != (size_t)-1) streams[s] = std::move(units[whole_at[s]]);
    std::vector<size_t> fallback;
    for (size_t r = 0; r < runs.size(); r++) {
        HostUnit& st = streams[runs[r].stream];
        HostUnit* run = &units[runs[r].first];
        size_t last = 0;
        if (!c.verdict(st, refs[runs[r].stream], run, joined[r], last)) { fallback.push_back(runs[r].stream); continue; }
        st.status = SWC_OK;
        st.aux_out = 0;
        st.in_consumed = (size_t)(run[last].in - st.in) + run[last].in_consumed;
        st.sum_valid = false;
        if ((c.sums >> st.sum_kind) & 1u) {   // the units' sums, combined: no pass over the joined output
            const bool crc = st.sum_kind == SWC_SUM_CRC32;
            bool valid = true;
            uint32_t sum = crc ? 0u : 1u;
            for (size_t k = 0; k <= last && valid; k++) {
                valid = run[k].sum_valid;
                sum = crc ? swc_crc32_combine(sum, (uint32_t)run[k].sum, run[k].out_size) : swc_adler32_combine(sum, (uint32_t)run[k].sum, run[k].out_size);
            }
            st.sum = sum;
            st.sum_valid = valid;
        }
    }
    if (!fallback.empty()) {
        std::vector<HostUnit> whole(fallback.size());
        for (size_t i = 0; i < fallback.size(); i++) whole[i] = std::move(streams[fallback[i]]);
        stat_add(c.fallbacks, (long long)fallback.size());
        rc = run_units(c.codec, whole);
        for (size_t i = 0; i < fallback.size(); i++) streams[fallback[i]] = std::move(whole[i]);
    }
    return rc;
}

int run_streams(int codec, std::vector<HostUnit>& streams, Cut cut) {
    if (cut == kCut && codec == SWC_CODEC_DEFLATE) return run_cut(deflate_runs(), streams);
    if (cut == kCut && codec == SWC_CODEC_LZMA2) return run_cut(lzma2_runs(), streams);
    return run_units(codec, streams);
}

int run_one(int codec, HostUnit& u, Cut cut) {
    std::vector<HostUnit> v(1);
    v[0] = std::move(u);
    int st = run_streams(codec, v, cut);
    u = std::move(v[0]);
    return st;
}

// run_one for a unit that is followed by unrelated data (the next members of a file, the next entries of a container):
// first with only `bound` bytes of input staged; the result stands if the unit decoded cleanly and ended inside them,
// anything else is decided by a second run over the whole tail -- so that a walk over M units stages O(file) bytes, not
// M times the rest of the file, and the outcome is the one the reference (which reads on from one reader) would have.
int run_one_bounded(int codec, HostUnit& u, size_t bound, Cut cut) {
    if (u.in_len <= bound) return run_one(codec, u, cut);
    HostUnit t = u;
    t.in_len = bound;
    int st = run_one(codec, t, cut);
    if (st != SWC_OK) return st;
    if (t.status == SWC_OK && t.in_consumed + 64 <= bound) { u = std::move(t); return SWC_OK; }
    return run_one(codec, u, cut);
}

}  // namespace swc
