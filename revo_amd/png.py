"""PNG decoding on the device (revo_png_* in include/revo_hip.h): a batch of PNG files (host bytes) is inflated and unfiltered
on the GPU straight into torch device tensors, in cv::imread's layouts (BGR8 colour, native uint16 depth).

Files the device decoder does not handle (interlaced, palette, < 8 bits, 16-bit colour) come back as UNSUPPORTED, malformed
ones as CORRUPT; the caller decides what to do with them (tum.GpuFrameSource decodes them on the CPU)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, vp

OK, INVALID_ARG, CAPACITY, UNSUPPORTED, CORRUPT = 0, -1, -5, -7, -8
BGR8, U16 = 0, 1


class PngInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32),
                ("interlace", C.c_int32), ("idat_bytes", C.c_uint64), ("raw_bytes", C.c_uint64)]


class PngJob(C.Structure):
    _fields_ = [("png", C.c_void_p), ("len", C.c_size_t), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("d_dst", C.c_void_p), ("dst_stride", C.c_size_t)]


def probe(data):
    """-> (code, PngInfo) of one file's bytes (host only)."""
    info = PngInfo()
    rc = _lib.lib().revo_png_probe(bytes(data), len(data), C.byref(info))
    return rc, info


def raw_bytes(width, height, fmt):
    """The inflated size of the largest file that decodes to this layout (RGBA8 for BGR8, gray16 for U16)."""
    return height * (1 + width * (4 if fmt == BGR8 else 2))


class GpuPngDecoder:
    """max_images files per submit, max_compressed_bytes of image data per submit, max_raw_bytes_per_image of inflated rows
    per image.  `cameraPyr` (an api.CameraPyr) picks its device; without it, `device`."""

    def __init__(self, max_images, max_compressed_bytes, max_raw_bytes_per_image, device=0, cameraPyr=None):
        import torch
        self.device = torch.device("cuda", cameraPyr.device if cameraPyr is not None and hasattr(cameraPyr, "device") else device)
        self.max_images = int(max_images)
        self._h = vp()
        with torch.cuda.device(self.device):
            check(_lib.lib().revo_png_decoder_create(cameraPyr._h if cameraPyr is not None else None, self.max_images,
                                                     int(max_compressed_bytes), int(max_raw_bytes_per_image), C.byref(self._h)))
        self._pending = {}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().revo_png_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, files, formats, outs, stream=None):
        """files: list of bytes; formats: one BGR8 / U16 per file (or one for all); outs: device tensors ([H,W,3] uint8 or
        [H,W] uint16, rows may be strided).  Returns a ticket for wait().  The file bytes may be reused at once."""
        import torch
        n = len(files)
        if isinstance(formats, int):
            formats = [formats] * n
        jobs = (PngJob * max(1, n))()
        keep = []
        for i, (f, fmt, o) in enumerate(zip(files, formats, outs)):
            b = bytes(f)
            keep.append(b)
            want = torch.uint8 if fmt == BGR8 else torch.uint16
            if o.dtype != want or o.device != self.device or o.dim() != (3 if fmt == BGR8 else 2):
                raise ValueError("output %d: needs a %s tensor on %s" % (i, want, self.device))
            if fmt == BGR8 and (o.shape[2] != 3 or o.stride(2) != 1 or o.stride(1) != 3):
                raise ValueError("output %d: BGR8 rows must be packed B,G,R pixels" % i)
            if fmt == U16 and o.stride(1) != 1:
                raise ValueError("output %d: u16 rows must be packed" % i)
            jobs[i].png = C.cast(C.c_char_p(b), C.c_void_p)
            jobs[i].len = len(b)
            jobs[i].format = int(fmt)
            jobs[i].height, jobs[i].width = int(o.shape[0]), int(o.shape[1])
            jobs[i].d_dst = o.data_ptr()
            jobs[i].dst_stride = o.stride(0) * o.element_size()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        t = C.c_uint64()
        check(_lib.lib().revo_png_decode_submit(self._h, n, jobs, C.c_void_p(s.cuda_stream), C.byref(t)))
        self._pending[t.value] = n
        return t.value

    def wait(self, ticket):
        """-> numpy int32 codes, one per file of the submit (OK, CORRUPT, UNSUPPORTED, INVALID_ARG)."""
        n = self._pending.pop(ticket)
        st = np.zeros(max(1, n), np.int32)
        check(_lib.lib().revo_png_decode_wait(self._h, C.c_uint64(ticket), st.ctypes.data_as(_lib.i32p)))
        return st[:n]

    def decode(self, files, fmt, width, height, outs=None, stream=None):
        """Decodes files (all of one format and size) into new tensors (or `outs`); -> (tensors, codes)."""
        import torch
        if outs is None:
            shape = (height, width, 3) if fmt == BGR8 else (height, width)
            outs = [torch.empty(shape, dtype=torch.uint8 if fmt == BGR8 else torch.uint16, device=self.device) for _ in files]
        codes = self.wait(self.submit(files, fmt, outs, stream))
        return outs, codes
