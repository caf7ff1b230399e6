"""The yardsticks of the per-method RX stage tests (include/mercury_stages.h; tests/test_stages_host.py, tests/test_gpu_stages.py).

* ctypes wrappers for the 13 entry points: host arrays in, host arrays out, every output buffer pre-filled with 0xA5 bytes so that a cell
  the kernel did not write cannot pass for a value; `call` returns the raw status for the refusal tests.
* plain numpy restatements of the integer and float32 stages, each written from the reference lines csrc/stages.hip cites.
  tests/test_stages_host.py proves them against the CPU oracle (and the reference's own objects where they were built) before they judge a
  kernel.
"""
import numpy as np

from mercury_amd.abi import PROTOTYPES

from demapper_csi_ref import same_bits  # noqa: F401  (shared with the tests)

MGPU_OK, MGPU_ERR_ARG = 0, 1            # include/mercury_gpu.h
SIGNATURES = PROTOTYPES["mercury_stages.h"]     # the 13 entry points, the context first
OFDM_ONLY = ("mgpu_automatic_gain_control", "mgpu_channel_estimator", "mgpu_restore_channel_amplitude", "mgpu_channel_equalizer",
             "mgpu_measure_variance", "mgpu_deframer", "mgpu_psk_demod")


_NOTHING = np.zeros(16, np.uint8)


def ptr(a):
    """the array's address; None stays the null pointer, an empty array gets a valid address all the same"""
    if a is None:
        return None
    return a.ctypes.data if a.size else _NOTHING.ctypes.data


def call(rx, name, *args):
    """the raw status of one entry point: arrays go in by address, None as a null pointer, integers as they are"""
    return getattr(rx.lib, name)(rx.h, *[ptr(a) if a is None or isinstance(a, np.ndarray) else int(a) for a in args])


def last_error(rx):
    return rx.lib.mgpu_last_error(rx.h).decode()


def blank(shape, dtype):
    out = np.empty(shape, dtype)
    out.view(np.uint8)[...] = 0xA5
    return out


def _in(a, dtype, width):
    a = np.ascontiguousarray(a, dtype)
    return a.reshape(-1, width) if width else a.reshape(a.shape[0], 0)


class Stages:
    """The 13 entry points on one context, F rows per call (F from the first array's shape); a status other than MGPU_OK raises."""

    def __init__(self, rx):
        self.rx, self.G = rx, rx.Nsymb * rx.Nc

    def _go(self, name, *args):
        self.rx._ck(call(self.rx, name, *args))

    def symbol_demod(self, x):
        x = _in(x, np.complex128, self.rx.Nofdm)
        out = blank((x.shape[0], self.rx.Nc), np.complex128)
        self._go("mgpu_symbol_demod", x, x.shape[0], out)
        return out

    def frame_grid(self, bb):
        """symbol_demod on whole frames: [F, Nsymb * Nofdm] -> [F, G]"""
        bb = _in(bb, np.complex128, self.rx.Nsymb * self.rx.Nofdm)
        return self.symbol_demod(bb).reshape(bb.shape[0], self.G)

    def agc(self, grid):
        g = _in(grid, np.complex128, self.G).copy()
        self._go("mgpu_automatic_gain_control", g, g.shape[0])
        return g

    def estimator(self, grid):
        g = _in(grid, np.complex128, self.G)
        out = blank(g.shape, np.complex128)
        self._go("mgpu_channel_estimator", g, g.shape[0], out)
        return out

    def restore(self, H):
        h = _in(H, np.complex128, self.G).copy()
        self._go("mgpu_restore_channel_amplitude", h, h.shape[0])
        return h

    def equalizer(self, grid, H):
        g, h = _in(grid, np.complex128, self.G), _in(H, np.complex128, self.G)
        assert g.shape == h.shape
        out = blank(g.shape, np.complex128)
        self._go("mgpu_channel_equalizer", g, h, g.shape[0], out)
        return out

    def variance(self, grid):
        g = _in(grid, np.complex128, self.G)
        out = blank(g.shape[0], np.float64)
        self._go("mgpu_measure_variance", g, g.shape[0], out)
        return out

    def deframer(self, grid):
        g = _in(grid, np.complex128, self.G)
        out = blank((g.shape[0], self.rx.nData), np.complex128)
        self._go("mgpu_deframer", g, g.shape[0], out)
        return out

    def _deint(self, name, x, dtype, bs):
        assert x.ndim == 2
        x = np.ascontiguousarray(x, dtype)
        out = blank(x.shape, dtype)
        self._go(name, x, x.shape[0], x.shape[1], bs, out)
        return out

    def deint_c128(self, x, bs):
        return self._deint("mgpu_deinterleaver_c128", x, np.complex128, bs)

    def deint_f32(self, x, bs):
        return self._deint("mgpu_deinterleaver_f32", x, np.float32, bs)

    def psk_demod(self, syms, variance_f):
        s = _in(syms, np.complex128, self.rx.nData)
        v = np.ascontiguousarray(variance_f, np.float32).reshape(-1)
        assert v.size == s.shape[0]
        out = blank((s.shape[0], self.rx.nBits), np.float32)
        self._go("mgpu_psk_demod", s, s.shape[0], v, out)
        return out

    def dispersal(self, bits):
        assert bits.ndim == 2
        b = np.ascontiguousarray(bits, np.uint8)
        out = blank(b.shape, np.uint8)
        self._go("mgpu_bit_energy_dispersal", b, b.shape[0], b.shape[1], out)
        return out

    def bit_to_byte(self, bits):
        assert bits.ndim == 2
        b = np.ascontiguousarray(bits, np.uint8)
        out = blank((b.shape[0], (b.shape[1] + 7) // 8), np.uint8)
        self._go("mgpu_bit_to_byte", b, b.shape[0], b.shape[1], out)
        return out

    def crc16(self, data):
        assert data.ndim == 2
        b = np.ascontiguousarray(data, np.uint8)
        out = blank(b.shape[0], np.uint16)
        self._go("mgpu_crc16_modbus_rtu", b, b.shape[0], b.shape[1], out)
        return out


# ---- the numpy restatements ---------------------------------------------------------------------------------------------------------
def deinterleave(x, bs):
    """deinterleaver (interleaver.cc:94-109) along the last axis: out[i*bs + j] = in[j*nb + i] for the nb = n // bs whole blocks, the
    n - nb*bs items behind them copied through. Items are moved, never computed on: any dtype, bit patterns kept."""
    x = np.asarray(x)
    n = x.shape[-1]
    nb = n // bs
    out = x.copy()
    head = x[..., : nb * bs].reshape(x.shape[:-1] + (bs, nb))          # [j][i] = in[j*nb + i]
    out[..., : nb * bs] = np.swapaxes(head, -1, -2).reshape(x.shape[:-1] + (nb * bs,))
    return out


def repack(dei, nReal, nVirtual, Pbits, N=1600):
    """the shortening re-pack of telecom_system.cc:1300-1308 (mercury_oracle.c:885-886) on one de-interleaved LLR row, in place order: the
    parity moves up behind the virtual bits (from the top down), then the virtual bits are copies of the first data bits (from the bottom up)"""
    out = np.zeros(N, np.float32)
    out[: dei.size] = dei
    for i in range(Pbits - 1, -1, -1):
        out[i + nReal + nVirtual] = out[i + nReal]
    for i in range(nVirtual):
        out[nReal + i] = out[i]
    return out


def bit_to_byte(bits):
    """bit_to_byte (misc.cc:107-130) along the last axis: LSB first, a trailing partial byte from the bits that are there"""
    b = np.asarray(bits).astype(np.uint8) & 1
    nbytes = (b.shape[-1] + 7) // 8
    out = np.zeros(b.shape[:-1] + (nbytes,), np.uint8)
    for q in range(b.shape[-1]):
        out[..., q // 8] |= b[..., q] << (q % 8)
    return out


def crc16(data):
    """CRC16_MODBUS_RTU_calc (crc16_modbus_rtu.cc:25-45) of every row: init 0xFFFF, reflected polynomial 0xA001; no bytes: 0xFFFF"""
    d = np.asarray(data).astype(np.uint32)
    crc = np.full(d.shape[:-1], 0xFFFF, np.uint32)
    for j in range(d.shape[-1]):
        crc = crc ^ (d[..., j] & 0xFF)
        for _ in range(8):
            crc = np.where(crc & 1, (crc >> 1) ^ 0xA001, crc >> 1)
    return crc.astype(np.uint16)


def dispersal(bits, scrambler):
    """bit_energy_dispersal (interleaver.cc:111-117): XOR with the mode's sequence"""
    b = np.asarray(bits)
    return (b ^ np.asarray(scrambler)[: b.shape[-1]].astype(b.dtype)).astype(b.dtype)


def psk_demod(syms, variance_f, constellation):
    """cl_psk::demod (psk.cc:278-326) on rows of symbols, one float variance per row -> float32 [rows, n * bps].
    The squared distances are summed in double and rounded to float; for every bit the minima start at D[0] / D[mask] and move on a strict
    `<`; LLR = (float(1) / variance) * (Dmin1 - Dmin0) in float; the bits of a symbol leave in reversed order."""
    s = np.atleast_2d(np.asarray(syms, np.complex128))
    var = np.asarray(variance_f, np.float32).reshape(-1)
    c = np.asarray(constellation, np.complex128)
    M = c.size
    bps = M.bit_length() - 1
    assert 1 << bps == M and var.size == s.shape[0]
    with np.errstate(all="ignore"):
        dr, di = s.real[..., None] - c.real, s.imag[..., None] - c.imag
        D = (dr * dr + di * di).astype(np.float32)                       # [rows, n, M]
        inv = (np.float32(1) / var)[:, None]
        out = np.zeros(s.shape + (bps,), np.float32)
        for k in range(bps):
            mask = 1 << k
            d0, d1 = D[..., 0].copy(), D[..., mask].copy()
            for j in range(M):
                if j & mask:
                    d1 = np.where(D[..., j] < d1, D[..., j], d1)
                else:
                    d0 = np.where(D[..., j] < d0, D[..., j], d0)
            llr = inv * (d1 - d0)
            assert llr.dtype == np.float32
            out[..., bps - 1 - k] = llr
    return out.reshape(s.shape[0], -1)
