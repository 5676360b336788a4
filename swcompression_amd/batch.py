"""Device-resident batches for the many-buffer launch (`swc_batch_decompress`).

PyTorch is used only as plumbing here: HBM allocations (`torch.empty(..., device='cuda')`), the
current HIP stream, and (in bench.py) `torch.distributed` for multi-GPU bookkeeping.  The decode itself
is the hand-written HIP kernels inside libswc_hip.so, reached through the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib

CODECS = {"deflate": 1, "lz4_block": 2, "lzma2": 3, "lzma": 4, "bzip2_block": 5, "delta": 6, "lz4_compress": 7, "deflate_compress": 8,
          "deflate_compress_dynamic": 9, "lzma2_compress": 10}

JOB_DTYPE = np.dtype([("in", "<u8"), ("in_len", "<u8"), ("out", "<u8"), ("out_cap", "<u8"), ("out_len", "<u8"),
                      ("in_consumed", "<u8"), ("status", "<i4"), ("aux", "<i4"), ("dict", "<u8"), ("dict_len", "<u8")])
assert JOB_DTYPE.itemsize == C.sizeof(_lib.SwcJob) == 72


def _align(x, a=16):
    return (x + a - 1) // a * a


class DeviceBatch:
    """`n_distinct` compressed units staged once in HBM and tiled `tile` times at DISTINCT device
    addresses (inputs are replicated, every job owns its own output range), as SURVEY.md section 8d asks for:
    nothing is served from the 256 MiB Infinity Cache by accident."""

    LZ4_LINKED, LZ4_STORED = 1, 2   # aux bits of an "lz4_block" job (include/swc_hip.h: swc_lz4_aux)
    DEFLATE_JOINED, DEFLATE_OPEN = 1, 2   # aux bits of a "deflate" job (swc_deflate_aux): the units of a stream cut at its flush points
    DEFLATE_LINKED = 4                    # ... together with DEFLATE_JOINED: the unit shares the history of the units in front of it
    LZMA2_OPEN = 0x100                    # aux bit of an "lzma2" job above its dictionary-size byte (swc_lzma2_aux): a unit that ends without the end marker

    def __init__(self, codec, units, caps, aux=None, extra=None, dict_values=None, tile=1, device="cuda:0", replicate_inputs=True,
                 select=None, dicts=None, prefixes=None, guard=0):
        """select = (lo, hi): the jobs are the units lo..hi-1 of the TILED unit list (list entry i is distinct unit i % n_distinct
        in replica i // n_distinct); default: the whole list of n_distinct * tile entries.
        LZ4 (tile = 1): dicts[i] = a prefix dictionary staged somewhere else (bytes or None); prefixes[i] = a prefix staged directly
        in front of job i's output (an adjacent prefix: history in place).  The output ranges follow each other in job order, so
        the head of a chain of LZ4_LINKED jobs -- of a run of DEFLATE_JOINED jobs -- owns the sum of the chain's capacities; guard = that many bytes of 0xA5 in front of
        every unlinked job's range (and its prefix) and behind the last one -- unwritten_intact() checks them.
        Deflate: aux=[...] holds the DEFLATE_* bits of every job -- DEFLATE_OPEN | (DEFLATE_JOINED on all but the head of a run) for units
        that stand alone, DEFLATE_JOINED | DEFLATE_LINKED for a unit that may refer to the 32,768 bytes in front of it (the units of a
        default-pigz or Z_SYNC_FLUSH stream); a job without DEFLATE_LINKED starts a new chain of shared history."""
        import torch
        self.torch = torch
        self.lib = _lib.load()
        if not self.lib.swc_device_available():
            raise RuntimeError("no usable gfx950 device: the MI355X engine has no CPU fallback")
        self.codec = CODECS[codec] if isinstance(codec, str) else int(codec)
        self.device = torch.device(device)
        nd = len(units)
        self.n_distinct = nd
        lo, hi = (0, nd * tile) if select is None else (int(select[0]), int(select[1]))
        self.tile = tile
        self.n = hi - lo
        lens = np.array([len(u) for u in units], dtype=np.uint64)
        caps = np.array(caps, dtype=np.uint64)
        in_sz = np.array([_align(int(x)) for x in lens], dtype=np.uint64)
        out_sz = np.array([_align(int(x)) for x in caps], dtype=np.uint64)
        in_off = np.concatenate([[0], np.cumsum(in_sz)[:-1]]).astype(np.uint64)
        in_round = int(in_sz.sum())
        host = np.zeros(in_round + 16, dtype=np.uint8)
        for u, o in zip(units, in_off):
            host[int(o):int(o) + len(u)] = np.frombuffer(u, dtype=np.uint8)
        idx = np.arange(lo, hi, dtype=np.int64)
        k_idx = (idx % nd).astype(np.int64) if nd else idx
        t_idx = (idx // nd).astype(np.uint64) if nd else idx.astype(np.uint64)
        t0 = int(t_idx.min()) if self.n else 0
        t1 = int(t_idx.max()) if self.n else 0
        in_tiles = (t1 - t0 + 1) if replicate_inputs else 1
        self.d_in = torch.empty(in_round * in_tiles + 16, dtype=torch.uint8, device=self.device)
        h = torch.from_numpy(host[:in_round])
        for t in range(in_tiles):
            self.d_in[t * in_round:(t + 1) * in_round].copy_(h)
        out_each = out_sz[k_idx]
        self._guard = int(guard)
        self._prefixes = None
        if dicts is not None or prefixes is not None or guard:
            assert tile == 1 and select is None
            aux_l = [0] * nd if aux is None else [int(a) for a in aux]
            placed = self.codec in (CODECS["deflate"], CODECS["lz4_block"])   # (bit 0 of any other codec's aux is no link)
            front = np.array([(0 if placed and aux_l[i] & self.LZ4_LINKED else int(guard)) + (_align(len(prefixes[i])) if prefixes is not None and prefixes[i] else 0)
                              for i in range(nd)], dtype=np.uint64)
            out_off = (np.concatenate([[0], np.cumsum(out_each + front)[:-1]]).astype(np.uint64) + front) if self.n else np.zeros(0, dtype=np.uint64)
            out_total = int((out_each + front).sum()) + int(guard)
        else:
            out_off = np.concatenate([[0], np.cumsum(out_each)[:-1]]).astype(np.uint64) if self.n else np.zeros(0, dtype=np.uint64)
            out_total = int(out_each.sum())
        self.d_out = torch.empty(out_total + 16, dtype=torch.uint8, device=self.device)
        if guard:
            self.d_out.fill_(0xA5)
        jobs = np.zeros(self.n, dtype=JOB_DTYPE)
        jobs["in"] = self.d_in.data_ptr() + ((t_idx - np.uint64(t0)) * np.uint64(in_round) if replicate_inputs else 0) + in_off[k_idx]
        jobs["in_len"] = lens[k_idx]
        jobs["out"] = self.d_out.data_ptr() + out_off
        jobs["out_cap"] = caps[k_idx]
        jobs["status"] = 902
        if aux is not None:
            jobs["aux"] = np.array(aux, dtype=np.int32)[k_idx]
        if extra is not None:
            jobs["dict_len"] = np.array(extra, dtype=np.uint64)[k_idx]
        if dict_values is not None:  # integer carried in the `dict` field (LZMA: dictionary size, BZip2: stored block CRC)
            jobs["dict"] = np.array(dict_values, dtype=np.uint64)[k_idx]
        if dicts is not None and any(d is not None for d in dicts):   # prefixes somewhere else: one more input buffer
            blob = b"".join(bytes(d) + bytes(_align(len(d)) - len(d)) for d in dicts if d is not None)
            self.d_dicts = torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).to(self.device)
            at = 0
            for i, d in enumerate(dicts):
                if d is not None:
                    jobs["dict"][i] = self.d_dicts.data_ptr() + at
                    jobs["dict_len"][i] = len(d)
                    at += _align(len(d))
        if prefixes is not None:
            self._prefixes = [None if p is None else bytes(p) for p in prefixes]
            for i, p in enumerate(self._prefixes):
                if p:
                    o = int(out_off[i]) - len(p)
                    self.d_out[o:o + len(p)].copy_(torch.from_numpy(np.frombuffer(p, dtype=np.uint8).copy()))
                    jobs["dict"][i] = self.d_out.data_ptr() + o
                    jobs["dict_len"][i] = len(p)
        self._out_off = out_off.astype(np.int64)
        self.unit_index = k_idx            # which distinct unit every job decodes
        self.caps = caps[k_idx]
        self.in_lens = lens[k_idx]
        self._jobs_host = jobs
        self.d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(self.device)
        ws = self.lib.swc_batch_workspace_bytes(self.codec, self.n, int(caps.max()) if nd else 0)
        self.d_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=self.device)
        self.ws_bytes = ws
        self._crc_buf = None
        self._crc_current = False   # _crc_buf holds the CRC-32 of what the latest launch wrote
        torch.cuda.synchronize(self.device)

    @property
    def total_in(self):
        return int(self.in_lens.sum())

    def launch(self, sync=False):
        """One launch over all jobs.  A Deflate batch whose CRCs have been asked for once (crc32_async() has allocated the
        buffer) keeps them current from then on: the launch goes through swc_batch_decompress_crc32_ws, whose copy kernel
        leaves the CRC-32 of every output in the buffer."""
        torch = self.torch
        opts = _lib.SwcBatchOpts(self.device.index if self.device.index is not None else -1,
                                 torch.cuda.current_stream(self.device).cuda_stream, 1 if sync else 0, 0)
        self._crc_current = False
        if self.codec == CODECS["deflate"] and self._crc_buf is not None:
            st = self.lib.swc_batch_decompress_crc32_ws(self.codec, self.d_jobs.data_ptr(), self.n, self.d_ws.data_ptr(),
                                                        self.ws_bytes, self._crc_buf.data_ptr(), C.byref(opts))
            self._crc_current = st == 0
        else:
            st = self.lib.swc_batch_decompress_ws(self.codec, self.d_jobs.data_ptr(), self.n, self.d_ws.data_ptr(),
                                                  self.ws_bytes, C.byref(opts))
        if st:
            raise RuntimeError("swc_batch_decompress failed with status %d" % st)

    def crc32(self):
        """CRC-32 of every job's output, computed on the device (swc_batch_crc32).  Returns a numpy uint32 array.  Always the
        standalone kernels over the bytes that lie in memory: an independent check of what a fused launch left in the buffer
        of crc32_async()."""
        torch = self.torch
        d = torch.empty(self.n, dtype=torch.int32, device=self.device)
        opts = _lib.SwcBatchOpts(self.device.index if self.device.index is not None else -1,
                                 torch.cuda.current_stream(self.device).cuda_stream, 1, 0)
        st = self.lib.swc_batch_crc32(self.d_jobs.data_ptr(), self.n, d.data_ptr(), C.byref(opts))
        if st:
            raise RuntimeError("swc_batch_crc32 failed with status %d" % st)
        return d.cpu().numpy().view(np.uint32)

    def crc32_async(self):
        """swc_batch_crc32 on the current stream, no synchronisation, result left on the device (bench.py: the CRC-32 of
        every gzip member is part of the timed step).  Returns at once when the buffer already belongs to the latest launch
        (launch() of a Deflate batch keeps it current once this method has allocated it); wipe_results() ends that."""
        torch = self.torch
        if self._crc_current:
            return
        if self._crc_buf is None:
            self._crc_buf = torch.empty(self.n, dtype=torch.int32, device=self.device)
        opts = _lib.SwcBatchOpts(self.device.index if self.device.index is not None else -1,
                                 torch.cuda.current_stream(self.device).cuda_stream, 0, 0)
        st = self.lib.swc_batch_crc32(self.d_jobs.data_ptr(), self.n, self._crc_buf.data_ptr(), C.byref(opts))
        if st:
            raise RuntimeError("swc_batch_crc32 failed with status %d" % st)

    CHECKSUMS = {"crc32": 1, "adler32": 2, "crc64": 3, "bzip2crc32": 4, "xxh32": 5}

    def checksum(self, kind):
        """Checksum `kind` (a key of CHECKSUMS, the names of the reference's CheckSums / XxHash32 functions) of every
        job's output, computed on the device (swc_batch_checksum).  Returns a numpy uint64 array."""
        torch = self.torch
        d = torch.empty(self.n, dtype=torch.int64, device=self.device)
        opts = _lib.SwcBatchOpts(self.device.index if self.device.index is not None else -1,
                                 torch.cuda.current_stream(self.device).cuda_stream, 1, 0)
        st = self.lib.swc_batch_checksum(self.CHECKSUMS[kind], self.d_jobs.data_ptr(), self.n, d.data_ptr(), C.byref(opts))
        if st:
            raise RuntimeError("swc_batch_checksum failed with status %d" % st)
        return d.cpu().numpy().view(np.uint64)

    def sha256(self):
        """SHA-256 of every job's output, computed on the device (swc_batch_sha256): one job per lane.  Returns a numpy uint8
        array of shape (n, 32), row i the digest of job i in the standard's byte order."""
        torch = self.torch
        d = torch.empty(max(self.n, 1) * 32, dtype=torch.uint8, device=self.device)
        opts = _lib.SwcBatchOpts(self.device.index if self.device.index is not None else -1,
                                 torch.cuda.current_stream(self.device).cuda_stream, 1, 0)
        st = self.lib.swc_batch_sha256(self.d_jobs.data_ptr(), self.n, d.data_ptr(), C.byref(opts))
        if st:
            raise RuntimeError("swc_batch_sha256 failed with status %d" % st)
        return d.cpu().numpy()[:self.n * 32].reshape(self.n, 32)

    def wipe_results(self):
        """Zeroes every job's output range, the result fields of the job records and the CRC buffer (bench.py: what is
        verified after the timed region must come from the last timed step, not from the warm-up).  The CRC buffer no longer
        belongs to a launch afterwards: the next crc32_async() without a launch computes it from what lies in memory."""
        self._crc_current = False
        self.d_out.zero_()
        jobs = self._jobs_host.copy()
        jobs["status"] = 902
        jobs["out_len"] = 0
        jobs["in_consumed"] = 0
        self.d_jobs.copy_(self.torch.from_numpy(jobs.view(np.uint8)).to(self.device))
        if self._crc_buf is not None:
            self._crc_buf.zero_()

    def results(self):
        """Structured numpy array of the job records after the launch (synchronises)."""
        self.torch.cuda.synchronize(self.device)
        return self.d_jobs.cpu().numpy().view(JOB_DTYPE)

    def output(self, i, n=None, moved=False):
        """The bytes job i left (n of them, default: as many as its record says).  moved=True: from where the job's `out` points
        after the launch -- the engine sets the `out` of an LZ4_LINKED / DEFLATE_JOINED job -- instead of where the batch put it."""
        r = self.results() if n is None or moved else None
        ln = int(min(r["out_len"][i], r["out_cap"][i])) if n is None else n
        o = int(r["out"][i]) - self.d_out.data_ptr() if moved else int(self._out_off[i])
        if not 0 <= o <= self.d_out.numel() - 16 - ln:
            raise RuntimeError("job %d: `out` points outside the batch's output buffer" % i)
        return self.d_out[o:o + ln].cpu().numpy().tobytes()

    def out_offset(self, i):
        """Where job i's `out` points after the launch, in bytes from where the batch put job i's own range."""
        return int(self.results()["out"][i]) - self.d_out.data_ptr() - int(self._out_off[i])

    def unwritten_intact(self):
        """A batch built with guard != 0: every byte of the output buffer outside what the job records say was produced still
        holds 0xA5, and every adjacent prefix its bytes."""
        r = self.results()
        blob = self.d_out.cpu().numpy()[:self.d_out.numel() - 16].copy()
        ok = True
        for i in range(self.n):
            o = int(r["out"][i]) - self.d_out.data_ptr()
            blob[o:o + int(min(r["out_len"][i], r["out_cap"][i]))] = 0xA5
            p = self._prefixes[i] if self._prefixes is not None else None
            if p:
                po = int(self._out_off[i]) - len(p)
                ok = ok and blob[po:po + len(p)].tobytes() == p
                blob[po:po + len(p)] = 0xA5
        return ok and bool((blob == 0xA5).all())


def bgzf_workspace_bytes(n_bytes, block_size=65280):
    return _lib.load().swc_bgzf_workspace_bytes(int(n_bytes), int(block_size))


def bgzf_archive(src, dst, block_size=65280, dynamic=False, workspace=None, dst_cap=None, sizes=True):
    """The device-resident BGZF writer (`swc_batch_bgzf_archive`): `src` and `dst` are torch uint8 tensors in HBM, `workspace` one
    of bgzf_workspace_bytes(src.numel(), block_size) bytes (allocated here when None), dst_cap the room in `dst` (default: all of
    it).  Returns (status, total, member_sizes): the swc_status of the call, the length of the file -- the length NEEDED for
    SWC_E_CAPACITY (901), when nothing has been written -- and, with sizes=True, a numpy uint64 array of the size of every member,
    the end-of-file member last."""
    import torch
    lib = _lib.load()
    n = int(src.numel())
    block_size = int(block_size) or 65280
    members = (n + block_size - 1) // block_size
    if workspace is None:
        workspace = torch.empty(max(bgzf_workspace_bytes(n, block_size), 16), dtype=torch.uint8, device=src.device)
    meta = torch.zeros(members + 2, dtype=torch.int64, device=src.device)
    dev = src.device
    opts = _lib.SwcBatchOpts(dev.index if dev.index is not None else -1, torch.cuda.current_stream(dev).cuda_stream, 1, 0)
    st = lib.swc_batch_bgzf_archive(src.data_ptr(), n, int(block_size), int(bool(dynamic)), dst.data_ptr(),
                                    int(dst.numel()) if dst_cap is None else int(dst_cap), meta.data_ptr(),
                                    meta.data_ptr() + 8 if sizes else None, workspace.data_ptr(), int(workspace.numel()), C.byref(opts))
    host = meta.cpu().numpy().view(np.uint64)
    return st, int(host[0]), (host[1:] if sizes else None)


def gzip_index_workspace_bytes(n_bytes, cap):
    return _lib.load().swc_gzip_index_workspace_bytes(int(n_bytes), int(cap))


def gzip_member_index(src, cap=None, workspace=None):
    """Every place a plain gzip member may start in `src`, a torch uint8 tensor in HBM (`swc_batch_gzip_index`: the candidate rule of
    include/swc_hip.h, swc_index_blocks kind 9).  cap: the most refs to write (default max(4096, bytes / 256)).  Returns (n, refs):
    the number of candidates found -- it may exceed cap -- and the first min(n, cap) refs as an (m, 4) int64 tensor that stays on the
    device: offset, comp_len, uncomp_len, and aux + (flags << 32) -- so a row whose last column is below 2^32 is usable (flags bit 0
    clear), and offset / comp_len / uncomp_len are what a DeviceBatch("deflate", ...) unit over `src` takes."""
    import torch
    lib = _lib.load()
    n_bytes = int(src.numel())
    cap = max(4096, n_bytes // 256) if cap is None else int(cap)
    if workspace is None:
        workspace = torch.empty(max(gzip_index_workspace_bytes(n_bytes, cap), 16), dtype=torch.uint8, device=src.device)
    refs = torch.empty((cap, 4), dtype=torch.int64, device=src.device)
    n = torch.zeros(1, dtype=torch.int64, device=src.device)
    dev = src.device
    opts = _lib.SwcBatchOpts(dev.index if dev.index is not None else -1, torch.cuda.current_stream(dev).cuda_stream, 1, 0)
    st = lib.swc_batch_gzip_index(src.data_ptr() if n_bytes else None, n_bytes, refs.data_ptr() if cap else None, cap, n.data_ptr(),
                                  workspace.data_ptr(), int(workspace.numel()), C.byref(opts))
    if st:
        raise RuntimeError("swc_batch_gzip_index failed with status %d" % st)
    found = int(n.item())
    return found, refs[:min(found, cap)]


def bzip2_index_workspace_bytes(n_bytes, cap):
    return _lib.load().swc_bzip2_index_workspace_bytes(int(n_bytes), int(cap))


def bzip2_mark_index(src, cap=None, workspace=None):
    """Every bit offset a bzip2 block or the end of a stream may start at in `src`, a torch uint8 tensor in HBM
    (`swc_batch_bzip2_index`: the mark rule of include/swc_hip.h, swc_index_blocks kind 10).  cap: the most refs to write (default
    max(4096, bytes / 4096)).  Returns (n, refs): the number of marks found -- it may exceed cap -- and the first min(n, cap) refs as an
    (m, 4) int64 tensor that stays on the device: offset and comp_len in bits, uncomp_len (0), and aux + (flags << 32) -- so a row
    whose last column is below 2^32 is a block (flags bit 0 clear) and the column is its stored CRC.  Such a row is a
    DeviceBatch("bzip2_block", ...) unit over the whole of `src`: extra = offset + 80 (the bit its body starts at), dict_value = aux.
    Marks are candidates: a unit counts only where a sequential walk arrives at its offset."""
    import torch
    lib = _lib.load()
    n_bytes = int(src.numel())
    cap = max(4096, n_bytes // 4096) if cap is None else int(cap)
    if workspace is None:
        workspace = torch.empty(max(bzip2_index_workspace_bytes(n_bytes, cap), 16), dtype=torch.uint8, device=src.device)
    refs = torch.empty((cap, 4), dtype=torch.int64, device=src.device)
    n = torch.zeros(1, dtype=torch.int64, device=src.device)
    dev = src.device
    opts = _lib.SwcBatchOpts(dev.index if dev.index is not None else -1, torch.cuda.current_stream(dev).cuda_stream, 1, 0)
    st = lib.swc_batch_bzip2_index(src.data_ptr() if n_bytes else None, n_bytes, refs.data_ptr() if cap else None, cap, n.data_ptr(),
                                   workspace.data_ptr(), int(workspace.numel()), C.byref(opts))
    if st:
        raise RuntimeError("swc_batch_bzip2_index failed with status %d" % st)
    found = int(n.item())
    return found, refs[:min(found, cap)]
