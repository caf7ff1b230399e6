"""What the two block-in, block-out IQ stages (mercury_amd.WidebandBlanker, mercury_amd.IqCorrector) refuse alike, at their smallest
blocks: the call checks and the device-tensor checks they share. Every refusal is pinned to its text and code, as the stages' own
sources and binding spelt them before they shared this code; it leaves the position where it was, and the next good call gives the
twin's bytes."""
import numpy as np
import pytest

from band_links import iq as _iq, last_error, rx as _rx, torch as _torch
from block_stage_cases import device_reports, same as _same
from mercury_amd import (IQC_REPORT_DTYPE, WBLANK_REPORT_DTYPE, IqCorrector, MgpuError, WidebandBlanker, host_iqc_process,
                         host_wblank_process)

pytestmark = pytest.mark.gpu

D, BLOCKS = 4, 4
STAGES = {"wblank": (WidebandBlanker, host_wblank_process, 64, WBLANK_REPORT_DTYPE, "blanker"),
          "iqc": (IqCorrector, host_iqc_process, 256, IQC_REPORT_DTYPE, "corrector")}
N_IN = "n_in must be a positive multiple of B, max_in at most, and the position stay below 2^62"
OVERLAP = "d_out must not overlap d_iq"
DEVICE_OUTPUT = "device output: device input, a contiguous tensor like it and a contiguous uint8 tensor [n_in / B, %d] or None"


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_a_refused_call_says_why_and_changes_nothing(stage):
    torch = _torch()
    make, twin, B, dtype, noun = STAGES[stage]
    x = _iq(np.random.default_rng(B), BLOCKS * B, "cf32")
    want = twin(x, D, block=B)
    st = make(_rx(), D, "cf32", block=B, max_in=BLOCKS * B)
    n = BLOCKS // 2 * B                                                 # a good call before the refusals, one after
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros(n, dtype=torch.complex64, device="cuda")
    d_strided = torch.zeros(2 * n, dtype=torch.complex64, device="cuda")[::2]
    d_reports = torch.zeros((BLOCKS // 2, dtype.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                            # the library works on its own stream
    first = st.process_raw(x[:n])                                       # the refusals meet a stage in mid-stream

    def refused(call, message, code, left):
        """call() raises MgpuError(message, code); `left`: what the context's last error then is (None: the binding refused, the library
        was not called)"""
        before = last_error(_rx())
        with pytest.raises(MgpuError) as e:
            call()
        assert (str(e.value), e.value.code) == (message, code)
        assert last_error(_rx()) == (before if left is None else left)
        assert st.status().position == n

    made_for = "the %s was made for IQ format 1, not 2" % noun
    refused(lambda: st.process_raw(x[:n].astype(np.complex128)), made_for, None, None)
    refused(lambda: st.process_raw(d_x[:n].to(torch.complex128), d_out), made_for, None, None)
    refused(lambda: st.process_raw(d_x[:n], d_strided), DEVICE_OUTPUT % dtype.itemsize, None, None)
    refused(lambda: st.process_raw(d_x[:n], d_out, d_reports[: BLOCKS // 2 - 1]), DEVICE_OUTPUT % dtype.itemsize, None, None)
    refused(lambda: st.process_raw(d_x[: 2 * B], d_x[B: 3 * B]), "mgpu error 1: " + OVERLAP, 1, OVERLAP)
    refused(lambda: st.process_raw(d_x[B: 3 * B], d_x[: 2 * B]), "mgpu error 1: " + OVERLAP, 1, OVERLAP)
    for bad in (x[: B - 1], x[: B + 1], np.concatenate([x, x[:B]])):    # less than a block, no multiple of B, more than max_in
        refused(lambda: st.process_raw(bad), "mgpu error 1: " + N_IN, 1, N_IN)
    refused(lambda: st.process_raw(d_x[: B - 1], d_out[: B - 1]), "mgpu error 1: " + N_IN, 1, N_IN)

    assert st.process_raw(d_x[n:], d_out, d_reports) == BLOCKS // 2
    st.rx.lib.mgpu_synchronize(st.rx.h, None)
    rest = (d_out.cpu().numpy(), device_reports(d_reports, BLOCKS // 2, dtype))
    assert _same((np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]])), want)
    st.close()
