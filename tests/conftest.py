import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a HIP (MI355X) device")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture(autouse=True)
def _device_for_test(request, monkeypatch):
    """Where a HIP device is present the package defaults to gpu:0. A test that is not marked
    ``gpu`` is a CPU test there too: it starts on the CPU, and the processes it starts see no
    device (the HIP runtime of this process is already up, so hiding them affects children
    only). A ``gpu`` test starts on gpu:0 whatever the test before it selected."""
    import torch
    if torch.cuda.is_available():
        import paddle_ray_amd as paddle
        if 'gpu' in request.keywords:
            paddle.set_device('gpu:0')
        else:
            paddle.set_device('cpu')
            # torch.cuda.device_count() reads the *_VISIBLE_DEVICES variables until the runtime
            # is initialised and then keeps its answer: fix it (at the real count) before the
            # devices are hidden, or a count of 0 would be kept and torch.manual_seed() would
            # no longer seed the GPU generator of the gpu tests that follow
            torch.cuda.init()
            torch.cuda.device_count()
            monkeypatch.setenv('HIP_VISIBLE_DEVICES', '')
            monkeypatch.setenv('CUDA_VISIBLE_DEVICES', '')
    yield


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no HIP device")
    for it in items:
        if 'gpu' in it.keywords:
            it.add_marker(skip)
