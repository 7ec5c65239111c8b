"""vorbis_aotuv_lancer_amd — MI355X-native batched Vorbis (aoTuV) encode path, plus a batched
device decoder (DecodeSetup, Decoder: Vorbis packets -> PCM; decode_ogg: .ogg files -> PCM; DeviceDemuxer: the Ogg demux of many files per call on the device; ChainSplitter, split_ogg_chain: the links of chained files; ResyncDemuxer, demux_ogg_resync: whole files that may be damaged; StreamSelector, select_vorbis_stream: the Vorbis stream of multiplexed files; OggFeed: the same for live streams, the next bytes of every stream per call; OggIndex: random sample
windows of many .ogg files, as PCM or cut into new .ogg files without a re-encode (OggCutter), of any mix of header classes with one_decoder=True (one MixedDecoder and one RangeStore with a class per stream); halfrate=True on any of them decodes at half the sample rate) and its mirror for whole
files (encode_ogg: PCM arrays of any lengths -> one .ogg each; plan_files: the schedule it follows).

Host-side mirror (Python) of the reference's per-block encode interface over the C ABI in
include/vorbis_mi355x.h.  PyTorch is used only as plumbing (device memory, streams,
torch.distributed); every transform runs in the hand-written gfx950 kernels of
libvorbis_mi355x.so.  There is no CPU fallback: importing works anywhere, but any compute
call raises if the HIP library or a GPU is missing.
"""
from ._lib import lib, LIB_PATH, COMPAT_LIB_PATH, VbmError, check  # noqa: F401
from .tables import window_table  # noqa: F401
from .mdct import MdctLookup, mdct_forward, window_mdct, window_fft_log  # noqa: F401

from .encoder import Setup, Encoder, FrontEnd, PacketInfo, batch_variants  # noqa: F401,E402
from .stream import header_packets, OggStream, OggMux, write_ogg, read_ogg, demux_ogg, DeviceDemuxer, DemuxBatch, demux_ogg_device, ChainSplitter, split_ogg_chain, ResyncDemuxer, demux_ogg_resync, StreamSelector, select_vorbis_stream, OggFeed, FeedResult, OggCutter, header_pages  # noqa: F401,E402
from .decoder import (DecodeSetup, Decoder, MixedDecoder, decode_ogg, decode_index, decode_index_device,  # noqa: F401,E402
                      decode_index_scan_host, RangeStore, LiveRangeStore, LiveAppend, OggIndex)  # noqa: F401,E402
from .files import encode_ogg, plan_files  # noqa: F401,E402

__all__ = ["Setup", "Encoder", "FrontEnd", "PacketInfo", "batch_variants", "header_packets", "OggStream", "OggMux", "write_ogg", "read_ogg", "demux_ogg", "DeviceDemuxer", "DemuxBatch", "demux_ogg_device", "ChainSplitter", "split_ogg_chain", "ResyncDemuxer", "demux_ogg_resync", "StreamSelector", "select_vorbis_stream", "OggFeed", "FeedResult", "OggCutter", "header_pages", "DecodeSetup", "Decoder", "MixedDecoder", "decode_ogg", "encode_ogg", "plan_files", "decode_index", "decode_index_device", "decode_index_scan_host", "RangeStore", "LiveRangeStore", "LiveAppend", "OggIndex", "lib", "LIB_PATH", "COMPAT_LIB_PATH", "VbmError", "check", "window_table",
           "MdctLookup", "mdct_forward", "window_mdct", "window_fft_log"]
