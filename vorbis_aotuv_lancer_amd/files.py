"""Whole files in batches, the encode-side mirror of decode_ogg: encode_ogg takes a list of PCM arrays of any lengths
and returns one .ogg per input.  Every file is driven as the reference application drives its one stream
(examples/encoder_example.c:179-236: write a chunk, hand out every ready block, at the end vorbis_analysis_wrote(0) and
hand out the rest); the files share the slots of one Encoder / FrontEnd / OggMux, a slot taking the next file when its
stream has delivered e_o_s.  plan_files is the schedule alone (pure Python, no device)."""
import numpy as np
import torch

from ._lib import VbmError
from .encoder import Setup, Encoder, FrontEnd
from .stream import OggMux


def plan_files(lengths, nslots, chunk=1024):
    """The delivery schedule of files with `lengths` samples over min(nslots, len(lengths)) slots -> (schedule, files).

    schedule: a list of steps
        ("write", {slot: n})   the next n samples of the file in each listed slot (one write per slot)
        ("drain",)             every slot hands out blocks until it has none
        ("finish", [slots])    vorbis_analysis_wrote(v, 0)
        ("restart", [slots])   the next file of each listed slot starts there
    files[slot]: the indices of the files that live in the slot, in the order they do (its generations).

    Per file it is the reference application's loop: `chunk` samples per write, the last one ragged, a drain after each
    write; finish in the step after the file's last write (the stream is drained by then), then a drain, which ends in
    e_o_s.  A zero-length file is finish alone.  Slot s starts with file s; a slot that has delivered e_o_s is
    restarted with the next file in list order (slots that end in the same step: in slot order)."""
    lengths = [int(n) for n in lengths]
    if any(n < 0 for n in lengths):
        raise ValueError("file lengths must not be negative")
    if nslots < 1 or chunk < 1:
        raise ValueError("nslots and chunk must be positive")
    nfiles = len(lengths)
    S = min(int(nslots), nfiles)
    files = [[s] for s in range(S)]
    left = {s: lengths[s] for s in range(S)}                 # live slots: samples of the slot's file not yet written
    upcoming = S
    schedule = []
    while left:
        ending = [s for s in sorted(left) if left[s] == 0]
        writes = {s: min(chunk, left[s]) for s in sorted(left) if left[s] > 0}
        if ending:
            schedule.append(("finish", ending))
        if writes:
            schedule.append(("write", writes))
        schedule.append(("drain",))
        for s, n in writes.items():
            left[s] -= n
        turned = []
        for s in ending:
            if upcoming < nfiles:
                files[s].append(upcoming)
                left[s] = lengths[upcoming]
                upcoming += 1
                turned.append(s)
            else:
                del left[s]
        if turned:
            schedule.append(("restart", turned))
    return schedule, files


MUX_ROUNDS = 8      # rounds per encode call of a drain = the most rows a stream has in one OggMux.mux call


class _Store:
    """every file's PCM in one device tensor: file i's channel c at base[i] + c * stride[i], n[i] floats; the strides are
    multiples of 4 floats, so every channel row starts on a 16-byte boundary"""

    def __init__(self, pcms, dev):
        if len({int(p.shape[0]) for p in pcms}) != 1:
            raise ValueError("all files need the same channel count")
        self.ch = int(pcms[0].shape[0])
        self.n = [int(p.shape[1]) for p in pcms]
        self.stride = [(n + 3) & ~3 for n in self.n]
        self.base = [0] * len(pcms)
        total = 0
        for i, st in enumerate(self.stride):
            self.base[i] = total
            total += self.ch * st
        host = np.zeros(max(total, 4), np.float32)
        on_device = []
        for i, p in enumerate(pcms):
            if isinstance(p, torch.Tensor) and p.is_cuda:
                on_device.append(i)
                continue
            a = p.numpy() if isinstance(p, torch.Tensor) else p
            host[self.base[i]:self.base[i] + self.ch * self.stride[i]].reshape(self.ch, self.stride[i])[:, :self.n[i]] = a
        self.data = torch.from_numpy(host).to(dev)           # the one upload
        for i in on_device:
            self.data[self.base[i]:self.base[i] + self.ch * self.stride[i]].view(self.ch, self.stride[i])[:, :self.n[i]] = \
                pcms[i].to(dev)


def _as_pcm(p, i):
    if isinstance(p, torch.Tensor):
        if p.dtype != torch.float32 or p.dim() != 2:
            raise ValueError(f"file {i}: PCM must be float32 [channels, samples]")
        return p.detach()
    a = np.asarray(p)
    if a.dtype != np.float32 or a.ndim != 2:
        raise ValueError(f"file {i}: PCM must be float32 [channels, samples]")
    return a


def _write_ragged(fe, store, slots, file_ids, at, vals):
    """one step's writes: every listed slot takes vals[k] samples of its file from at[k] on, in one call"""
    fe.write_ragged(slots, store.data, [store.base[i] + a for i, a in zip(file_ids, at)], vals,
                    [store.stride[i] for i in file_ids])


def encode_ogg(pcms, rate, quality=0.5, bitrate=None, chunk=1024, max_streams=4096, serialnos=None, comments=()):
    """PCM of whole files -> .ogg bytes, one per input: the mirror of decode_ogg.

    pcms: a sequence of float32 [channels, n_i] arrays (numpy or torch, host or device), all with the same channel
    count, of any lengths (0 included).  rate, quality / bitrate: the class, as for Setup (FileNotFoundError for one
    without a mode pack).  serialnos: one per file (default: the file's index).  comments: for every file.

    File i's bytes are what write_ogg makes of the packets of ONE stream that is given file i as the reference
    application gives it (`chunk` samples per write and a drain after each, then the end and a drain), with
    serialnos[i] and the comments: they do not depend on the slot the file ran in, on max_streams, or on what else is
    in the list.  The files are uploaded once; min(len(pcms), max_streams) slots run plan_files' schedule with
    FrontEnd.write_ragged straight from that store, and OggMux pages the rounds' rows on the device."""
    return _run_files(pcms, rate, quality, bitrate, chunk, max_streams, serialnos, comments, _write_ragged)


def _run_files(pcms, rate, quality, bitrate, chunk, max_streams, serialnos, comments, write):
    """encode_ogg with the step's write left to `write` (tools/bench_encode_files.py measures other ways to deliver the
    same samples)"""
    pcms = [_as_pcm(p, i) for i, p in enumerate(pcms)]
    nfiles = len(pcms)
    if serialnos is None:
        serialnos = list(range(nfiles))
    serialnos = [int(x) for x in serialnos]
    if len(serialnos) != nfiles:
        raise ValueError("one serial number per file")
    if max_streams < 1 or chunk < 1:
        raise ValueError("max_streams and chunk must be positive")
    if nfiles == 0:
        return []
    ch = int(pcms[0].shape[0])
    setup = Setup(ch, rate, quality, bitrate)
    dev = torch.device("cuda", torch.cuda.current_device())
    S = min(nfiles, int(max_streams))
    enc = fe = mux = None
    try:
        enc = Encoder(setup, S)
        fe = FrontEnd(enc)
        # a drained stream carries less than two long blocks into its next write (csrc/capi_frontend.cpp)
        if chunk > fe.capacity - 2 * setup.blocksizes[1]:
            raise ValueError(f"chunk must be at most {fe.capacity - 2 * setup.blocksizes[1]} samples for this class")
        store = _Store(pcms, dev)
        schedule, files = plan_files(store.n, S, chunk)
        gen, at = [0] * S, [0] * S
        ended = [False] * S
        out = [[] for _ in range(nfiles)]

        def current(s):
            return files[s][gen[s]]

        mux = OggMux(setup, S, enc.max_packet_bytes, serialnos=[serialnos[current(s)] for s in range(S)],
                     comments=comments, max_rows_per_stream=MUX_ROUNDS, device=dev)
        for s, pages in enumerate(mux.start()):
            out[current(s)].append(pages)

        for step in schedule:
            if step[0] == "write":
                slots = list(step[1])
                write(fe, store, slots, [current(s) for s in slots], [at[s] for s in slots], [step[1][s] for s in slots])
                for s in slots:
                    at[s] += step[1][s]
            elif step[0] == "drain":
                while True:
                    info, packets, nbytes, counts = fe.encode_rounds(min_rounds=MUX_ROUNDS, max_rounds=MUX_ROUNDS,
                                                                     cap_blocks=S * MUX_ROUNDS, device=dev)
                    if not counts:
                        break
                    for s in info["stream"][info["eos"] != 0]:
                        ended[int(s)] = True
                    # no flush, ever: the e_o_s packet completes its stream's last page (csrc/ogg_mux.h), and a flush
                    # would cut the pages of every other stream short
                    data, offsets, status = mux.mux(info, packets, nbytes)
                    offsets, status = offsets.cpu().numpy(), status.cpu().numpy()
                    if status.any():
                        bad = int(np.flatnonzero(status)[0])
                        raise VbmError(f"Ogg paging failed (VBM_MUX status {int(status[bad])} in slot {bad})")
                    raw = data[:int(offsets[S])].cpu().numpy().tobytes()
                    for s in np.flatnonzero(np.diff(offsets)):
                        out[current(s)].append(raw[offsets[s]:offsets[s + 1]])
            elif step[0] == "finish":
                fe.finish(step[1])
            else:
                slots = step[1]
                if not all(ended[s] for s in slots):
                    raise VbmError("a stream was drained after its end without delivering e_o_s")
                fe.restart_streams(slots)
                for s in slots:
                    gen[s] += 1
                    at[s] = 0
                    ended[s] = False
                for s, pages in zip(slots, mux.start(slots, serialnos=[serialnos[current(s)] for s in slots])):
                    out[current(s)].append(pages)
        if not all(ended):
            raise VbmError("a stream was drained after its end without delivering e_o_s")
        return [b"".join(parts) for parts in out]
    finally:
        if mux is not None:
            mux.close()
        if fe is not None:
            fe.close()
        if enc is not None:
            enc.close()
        setup.close()
