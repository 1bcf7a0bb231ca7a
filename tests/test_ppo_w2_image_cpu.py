"""The W2 image behind the chunk squares of the PPO `grad` buffer (csrc/ppo.hip, W2IMG_OFF): its size and alignment as
ppo_grad_floats() states them.  The library loads without a GPU (tests/test_abi_cpu.py)."""
import ctypes

from oracle import ppo_oracle as PO

NH, HS = 128, 129                              # W2 rows, the gradient kernel's LDS row stride
IMAGE = NH * HS                                # 16,512 words (a multiple of 4 already)
RED_BLOCKS = (PO.NPARAM + 5 + 127) // 128      # k_reduce_partials workgroups = chunk squares


def _grad_floats():
    from omniisaacgymenvs_loop_amd import _capi
    return ctypes.CDLL(_capi.LIB_PATH).ppo_grad_floats()


def test_grad_buffer_holds_the_image():
    assert IMAGE == 16512 and IMAGE % 4 == 0
    assert _grad_floats() >= PO.NPARAM + 8 + RED_BLOCKS + IMAGE


def test_image_starts_on_a_16_byte_boundary():
    start = _grad_floats() - IMAGE             # the image is the last floats of the buffer
    assert start >= PO.NPARAM + 8 + RED_BLOCKS
    assert start % 4 == 0
