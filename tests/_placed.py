"""Placement harness of the GPU tier: a batch whose inputs, outputs, prefixes and workspace lie at CHOSEN residues mod 16, every one of
them between guard bytes, and a verify() that compares whole buffers -- so that a store outside a job's range, a launch that leaves
its workspace, a kernel that writes to its input or to the IN fields of a job record cannot pass.  TEST INFRASTRUCTURE ONLY.

include/swc_hip.h states one alignment rule for the pointers of a job (`out` of the Deflate encoders: 4 bytes); every other placement
is in contract.  swcompression_amd.batch.DeviceBatch rounds every offset up to 16 and stays as it is; this module reuses its record
layout and codec numbers."""
import ctypes as C

import numpy as np

from swcompression_amd import _lib
from swcompression_amd.batch import CODECS, JOB_DTYPE

WS_GUARD = 4096
IN_FIELDS = ("in", "in_len", "out", "out_cap", "dict", "dict_len")
# aux bits include/swc_hip.h documents as OUT: SWC_DEFLATE_OPEN of a Deflate job; the whole field of a bzip2 block job, which the
# engine does not read and leaves holding the CRC-32 of the block's output -- verify() compares it with the expectation's aux_out
AUX_OUT = {CODECS["deflate"]: 2, CODECS["bzip2_block"]: -1}
CHECKSUMS = {"crc32": 1, "adler32": 2, "crc64": 3, "bzip2crc32": 4, "xxh32": 5}


def _up16(x):
    return (x + 15) // 16 * 16


class PlacedBatch:
    def __init__(self, codec, units, caps, in_res, out_res, aux=None, extra=None, dict_values=None, dicts=None, prefixes=None, guard=64,
                 fill=0xA5, in_place=None, same=None, device="cuda:0"):
        """Unit i's input starts at a device address of residue in_res[i] mod 16, its output range at residue out_res[i], both with at
        least `guard` bytes of `fill` on either side in buffers prefilled with `fill`.  dicts[i]: an LZ4 prefix somewhere else (in the
        input buffer, at a residue of its own); prefixes[i]: an LZ4 prefix directly in front of the output.  in_place[i] (Delta): the
        input lies where the output goes, `in` == `out`, at out_res[i].  same[i]: a key -- jobs with equal keys hold the same unit
        and must report the same status, lengths and bytes wherever they lie."""
        import torch
        self.torch = torch
        self.lib = _lib.load()
        if not self.lib.swc_device_available():
            raise RuntimeError("no usable gfx950 device")
        self.codec = CODECS[codec] if isinstance(codec, str) else int(codec)
        self.device = torch.device(device)
        n = self.n = len(units)
        self.units = [bytes(u) for u in units]
        self.caps = [int(c) for c in caps]
        self.in_res, self.out_res = [int(r) for r in in_res], [int(r) for r in out_res]
        assert len(self.caps) == len(self.in_res) == len(self.out_res) == n
        assert all(0 <= r < 16 for r in self.in_res + self.out_res)
        self.fill, self.guard = int(fill), int(guard)
        self.same = list(range(n)) if same is None else list(same)
        in_place = [False] * n if in_place is None else [bool(x) for x in in_place]
        self.in_place = in_place
        dicts = [None] * n if dicts is None else [None if d is None else bytes(d) for d in dicts]
        prefixes = [None] * n if prefixes is None else [bytes(p) if p else None for p in prefixes]
        self.prefixes = prefixes
        # --- inputs (and the prefixes that lie somewhere else)
        at, self.in_off, dict_off = 0, [0] * n, [None] * n
        for i, u in enumerate(self.units):
            if not in_place[i]:
                self.in_off[i] = _up16(at + guard) + self.in_res[i]
                at = self.in_off[i] + len(u)
            if dicts[i] is not None:
                dict_off[i] = _up16(at + guard) + (self.in_res[i] + 7) % 16
                at = dict_off[i] + len(dicts[i])
        in_host = np.full(_up16(at + guard) + 16, self.fill, dtype=np.uint8)
        for i, u in enumerate(self.units):
            if not in_place[i]:
                in_host[self.in_off[i]:self.in_off[i] + len(u)] = np.frombuffer(u, dtype=np.uint8)
            if dicts[i] is not None:
                in_host[dict_off[i]:dict_off[i] + len(dicts[i])] = np.frombuffer(dicts[i], dtype=np.uint8)
        # --- outputs (and the prefixes in front of them)
        at, self.out_off = 0, [0] * n
        for i in range(n):
            plen = len(prefixes[i]) if prefixes[i] else 0
            self.out_off[i] = _up16(at + guard + plen) + self.out_res[i]
            at = self.out_off[i] + self.caps[i]
        out_host = np.full(_up16(at + guard) + 16, self.fill, dtype=np.uint8)
        for i in range(n):
            if prefixes[i]:
                o = self.out_off[i] - len(prefixes[i])
                out_host[o:o + len(prefixes[i])] = np.frombuffer(prefixes[i], dtype=np.uint8)
            if in_place[i]:
                assert len(self.units[i]) <= self.caps[i]
                out_host[self.out_off[i]:self.out_off[i] + len(self.units[i])] = np.frombuffer(self.units[i], dtype=np.uint8)
        self.in_host, self.out_host = in_host, out_host
        self.d_in = torch.from_numpy(in_host).to(self.device)
        self.d_out = torch.from_numpy(out_host).to(self.device)
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0
        # --- the workspace: exactly swc_batch_workspace_bytes, 16-byte aligned, 4 KiB of fill on either side
        self.ws_bytes = int(self.lib.swc_batch_workspace_bytes(self.codec, n, max(self.caps) if n else 0))
        self.d_ws = torch.full((WS_GUARD + self.ws_bytes + WS_GUARD,), self.fill, dtype=torch.uint8, device=self.device)
        assert self.d_ws.data_ptr() % 16 == 0
        # --- the job records
        jobs = np.zeros(n, dtype=JOB_DTYPE)
        for i in range(n):
            jobs["out"][i] = self.d_out.data_ptr() + self.out_off[i]
            jobs["in"][i] = jobs["out"][i] if in_place[i] else self.d_in.data_ptr() + self.in_off[i]
            if dicts[i] is not None:
                jobs["dict"][i], jobs["dict_len"][i] = self.d_in.data_ptr() + dict_off[i], len(dicts[i])
            if prefixes[i]:
                jobs["dict"][i], jobs["dict_len"][i] = jobs["out"][i] - np.uint64(len(prefixes[i])), len(prefixes[i])
        jobs["in_len"] = [len(u) for u in self.units]
        jobs["out_cap"] = self.caps
        jobs["status"] = 902
        if aux is not None:
            jobs["aux"] = np.array(aux, dtype=np.int32)
        if extra is not None:
            jobs["dict_len"] = np.array(extra, dtype=np.uint64)
        if dict_values is not None:
            jobs["dict"] = np.array(dict_values, dtype=np.uint64)
        assert (jobs["in"] % 16 == np.where(in_place, self.out_res, self.in_res)).all() and (jobs["out"] % 16 == self.out_res).all()
        self.jobs_host = jobs
        self.d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(self.device)
        self.d_crc = None
        torch.cuda.synchronize(self.device)

    def residues_launched(self):
        """(set of input residues, set of output residues) of the device addresses in the job records."""
        return set(int(x) for x in self.jobs_host["in"] % 16), set(int(x) for x in self.jobs_host["out"] % 16)

    def _opts(self):
        return _lib.SwcBatchOpts(self.device.index if self.device.index is not None else -1,
                                 self.torch.cuda.current_stream(self.device).cuda_stream, 1, 0)

    def launch(self, crc=False, workspace=True):
        """swc_batch_decompress_ws with the exact workspace size; crc=True: swc_batch_decompress_crc32_ws; workspace=False:
        swc_batch_decompress (LZ4: the lane decoder)."""
        opts = self._opts()
        ws = self.d_ws.data_ptr() + WS_GUARD
        if crc:
            self.d_crc = self.torch.zeros(max(self.n, 1), dtype=self.torch.int32, device=self.device)
            st = self.lib.swc_batch_decompress_crc32_ws(self.codec, self.d_jobs.data_ptr(), self.n, ws, self.ws_bytes,
                                                        self.d_crc.data_ptr(), C.byref(opts))
        elif workspace:
            st = self.lib.swc_batch_decompress_ws(self.codec, self.d_jobs.data_ptr(), self.n, ws, self.ws_bytes, C.byref(opts))
        else:
            st = self.lib.swc_batch_decompress(self.codec, self.d_jobs.data_ptr(), self.n, C.byref(opts))
        assert st == 0, "the launch failed with status %d" % st
        self.torch.cuda.synchronize(self.device)
        self.res = self.d_jobs.cpu().numpy().view(JOB_DTYPE).copy()
        self.out_got = self.d_out.cpu().numpy().copy()

    def fused_crc32(self):
        return self.d_crc.cpu().numpy().view(np.uint32)[:self.n]

    def checksum(self, kind):
        d = self.torch.zeros(max(self.n, 1), dtype=self.torch.int64, device=self.device)
        opts = self._opts()
        st = self.lib.swc_batch_checksum(CHECKSUMS[kind], self.d_jobs.data_ptr(), self.n, d.data_ptr(), C.byref(opts))
        assert st == 0, "swc_batch_checksum %s failed with status %d" % (kind, st)
        return d.cpu().numpy().view(np.uint64)[:self.n]

    def crc32(self):
        d = self.torch.zeros(max(self.n, 1), dtype=self.torch.int32, device=self.device)
        opts = self._opts()
        st = self.lib.swc_batch_crc32(self.d_jobs.data_ptr(), self.n, d.data_ptr(), C.byref(opts))
        assert st == 0, "swc_batch_crc32 failed with status %d" % st
        return d.cpu().numpy().view(np.uint32)[:self.n]

    def where(self, i):
        return "job %d (in %% 16 = %d, out %% 16 = %d)" % (i, self.in_res[i] if not self.in_place[i] else self.out_res[i], self.out_res[i])

    def produced(self, i):
        """The bytes job i left: [out, out + min(out_len, out_cap))."""
        ln = int(min(self.res["out_len"][i], self.caps[i]))
        return self.out_got[self.out_off[i]:self.out_off[i] + ln].tobytes()

    def _owner(self, off):
        """Which job's surroundings a byte of the output buffer belongs to: for the message of a stray write."""
        best = max((i for i in range(self.n) if self.out_off[i] - self.guard - 16 <= off), key=lambda i: self.out_off[i], default=0)
        return "%s, offset %d from its `out` (capacity %d)" % (self.where(best), off - self.out_off[best], self.caps[best]) if self.n else "offset %d" % off

    def verify(self, expected):
        """expected[i] (a _placement_cases.Case, or anything with its four attributes): .status; .out_len / .in_consumed, None where the
        oracle has no word on them; .data, the bytes of the whole output (a job that ends with SWC_E_CAPACITY holds their first
        out_cap), None where they are not known beforehand (an encoder: produced(i) hands them to the test).  Asserts, each message
        naming the job, both residues and the first offending offset: status and lengths; ONE comparison of the whole output buffer
        with an image -- the fill everywhere, the expected bytes at [out, out + min(out_len, cap)); masked are only
        [out + min(out_len, cap), out + cap) of a job, and the whole range of a job that failed with anything but 901 or whose bytes
        are unknown; the input buffer unchanged; both workspace guards; the IN fields of the records and, where the expectation names it, the OUT value of `aux`; equal results for equal units."""
        assert len(expected) == self.n
        r = self.res
        image = self.out_host.copy()
        got = self.out_got.copy()
        for i, e in enumerate(expected):
            w = self.where(i)
            st, ol, ic = int(r["status"][i]), int(r["out_len"][i]), int(r["in_consumed"][i])
            assert st == e.status, "%s: status %d, expected %d" % (w, st, e.status)
            if e.out_len is not None:
                assert ol == e.out_len, "%s: out_len %d, expected %d" % (w, ol, e.out_len)
            if e.in_consumed is not None:
                assert ic == e.in_consumed, "%s: in_consumed %d, expected %d" % (w, ic, e.in_consumed)
            o, cap = self.out_off[i], self.caps[i]
            if st not in (0, 901) or e.data is None:
                got[o:o + cap] = image[o:o + cap]          # no contract covers these bytes: masked
                continue
            ln = min(ol, cap)
            assert len(e.data) >= ln, "%s: out_len %d, the expectation has %d bytes" % (w, ol, len(e.data))
            image[o:o + ln] = np.frombuffer(e.data[:ln], dtype=np.uint8)
            got[o + ln:o + cap] = image[o + ln:o + cap]    # behind what was produced, inside the capacity: masked
        bad = np.nonzero(got != image)[0]
        if len(bad):
            off = int(bad[0])
            raise AssertionError("output buffer differs from the expected image at %d places, first: %s, holds 0x%02x, expected 0x%02x"
                                 % (len(bad), self._owner(off), int(got[off]), int(image[off])))
        # the inputs: byte-identical to what was uploaded
        in_got = self.d_in.cpu().numpy()
        bad = np.nonzero(in_got != self.in_host)[0]
        if len(bad):
            off = int(bad[0])
            i = max((k for k in range(self.n) if self.in_off[k] - self.guard - 16 <= off), key=lambda k: self.in_off[k], default=0)
            raise AssertionError("input buffer changed at %d places, first: %s, offset %d from its `in`" % (len(bad), self.where(i), off - self.in_off[i]))
        # the workspace guards
        for name, part, base in (("in front of", self.d_ws[:WS_GUARD], -WS_GUARD), ("behind", self.d_ws[WS_GUARD + self.ws_bytes:], self.ws_bytes)):
            bad = np.nonzero(part.cpu().numpy() != self.fill)[0]
            assert not len(bad), "the launch wrote %s its workspace of %d bytes: first at offset %d" % (name, self.ws_bytes, base + int(bad[0]))
        # the IN fields of the job records
        for f in IN_FIELDS:
            bad = np.nonzero(r[f] != self.jobs_host[f])[0]
            assert not len(bad), "%s: field `%s` of the job record changed" % (self.where(int(bad[0])), f)
        keep = ~np.int32(AUX_OUT.get(self.codec, 0))
        bad = np.nonzero((r["aux"] & keep) != (self.jobs_host["aux"] & keep))[0]
        assert not len(bad), "%s: IN bits of `aux` changed" % self.where(int(bad[0]))
        for i, e in enumerate(expected):
            want = getattr(e, "aux_out", None)
            if want is not None:
                assert int(r["aux"][i]) == want, "%s: aux 0x%08x, expected 0x%08x" % (self.where(i), int(r["aux"][i]) & 0xFFFFFFFF, want & 0xFFFFFFFF)
        # residue independence
        first = {}
        for i in range(self.n):
            k = first.setdefault(self.same[i], i)
            if k != i:
                for f in ("status", "out_len", "in_consumed"):
                    assert int(r[f][i]) == int(r[f][k]), "%s: %s %d, but %d at %s" % (self.where(i), f, int(r[f][i]), int(r[f][k]), self.where(k))
                if int(r["status"][i]) in (0, 901):
                    assert self.produced(i) == self.produced(k), "%s: bytes differ from those at %s" % (self.where(i), self.where(k))
