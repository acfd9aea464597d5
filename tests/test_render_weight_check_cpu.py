"""Host logic of the decoder weight check in front of ia_render_rays (hipops._render_weights_checked) without a GPU: the bound, the
gains, and the cache -- one device read per version of the weight tensors, none on the cached path, none while a stream captures."""
import math

import pytest
import torch

from invertavatar_amd import hipops


@pytest.fixture
def reads(monkeypatch):
    """Counts the device reads and empties the cache."""
    calls = []
    real = hipops._render_weight_maxima

    def counted(w0, w1):
        calls.append(1)
        return real(w0, w1)
    monkeypatch.setattr(hipops, '_render_weight_maxima', counted)
    monkeypatch.setattr(hipops, '_render_weight_checks', {})
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    return calls


def _weights(staged0=1.0, staged1=1.0, lr=1.0):
    """(w0, w1) whose largest staged entries are the given values at lr_multiplier ``lr``."""
    w0, w1 = torch.full((64, 32), 0.01), torch.full((33, 64), 0.01)
    w0[5, 7] = -staged0 * math.sqrt(32.0) / math.log2(math.e) / lr
    w1[9, 3] = staged1 * math.sqrt(64.0) / lr
    w1[0, :] = 1e4            # the density row is not staged as a pair: it may be anything
    return w0, w1


def test_bound_and_gains(reads):
    for lr in (1.0, 0.5, 2.0):
        hipops._render_weights_checked(*_weights(15.5, 15.5, lr), lr)
        for s0, s1 in ((16.0, 1.0), (1.0, 16.0), (15.995, 1.0), (float('inf'), 1.0), (1.0, 1e30)):
            with pytest.raises(RuntimeError, match='15.99') as err:
                hipops._render_weights_checked(*_weights(s0, s1, lr), lr)
            assert ('w0 is' if s0 > 15.9 else 'w1 is') in str(err.value)
    # the same tensors at another lr_multiplier: judged again, not read again
    w0, w1 = _weights(10.0, 10.0, 1.0)
    n = len(reads)
    hipops._render_weights_checked(w0, w1, 1.0)
    with pytest.raises(RuntimeError, match='15.99'):
        hipops._render_weights_checked(w0, w1, 2.0)
    assert len(reads) == n + 1
    nan = _weights()
    nan[0][0, 0] = float('nan')
    with pytest.raises(RuntimeError, match='15.99'):
        hipops._render_weights_checked(*nan, 1.0)


def test_one_read_per_version(reads):
    w0, w1 = _weights(3.0, 3.0)
    for _ in range(5):
        hipops._render_weights_checked(w0, w1, 1.0)
    assert len(reads) == 1
    w1.mul_(2.0)                                    # in place: same pointer, new version
    hipops._render_weights_checked(w0, w1, 1.0)
    hipops._render_weights_checked(w0, w1, 1.0)
    assert len(reads) == 2
    w0.mul_(8.0)
    for _ in range(2):                              # a refused version stays refused without another read
        with pytest.raises(RuntimeError, match='w0'):
            hipops._render_weights_checked(w0, w1, 1.0)
    assert len(reads) == 3
    other = w0.clone().mul_(0.1)                    # another tensor
    hipops._render_weights_checked(other, w1, 1.0)
    assert len(reads) == 4
    many = [torch.zeros(64, 32) for _ in range(200)]
    for t in many:                                  # the cache stays small
        hipops._render_weights_checked(t, w1, 1.0)
    assert len(hipops._render_weight_checks) <= 64 and len(reads) == 204


def test_a_new_tensor_at_a_freed_address_is_read_again(reads):
    w1 = _weights()[1]
    seen = set()
    for k in range(50):                             # the allocator hands the freed block out again: same pointer, same version
        w0 = torch.full((64, 32), 0.01)
        seen.add(w0.data_ptr())
        if k % 2:
            w0[0, 0] = 1e3
            with pytest.raises(RuntimeError, match='w0'):
                hipops._render_weights_checked(w0, w1, 1.0)
        else:
            w0[0, 0] = 0.02
            hipops._render_weights_checked(w0, w1, 1.0)
        del w0
    assert len(reads) == 50 and len(seen) < 50


def test_no_read_while_capturing(reads, monkeypatch):
    known, new = _weights(3.0, 3.0), _weights(99.0, 3.0)
    hipops._render_weights_checked(*known, 1.0)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    hipops._render_weights_checked(*known, 1.0)     # cached: judged as before
    hipops._render_weights_checked(*new, 1.0)       # unknown: a read would break the capture, so nothing is read or judged
    assert len(reads) == 1 and len(hipops._render_weight_checks) == 1
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    with pytest.raises(RuntimeError, match='w0'):
        hipops._render_weights_checked(*new, 1.0)
