"""Ours, not the reference's: a fixed seed before every staged reference test, in the suite's run and in
tests/test_reference_suite_gpu.py's subprocess run alike.  The staged tests draw their inputs unseeded (torch.rand /
torch.randn / numpy / random); test_barycentrics* solve 3x3 systems built from such draws, and an ill-conditioned draw
fails their tolerance now and then whatever library is underneath.  Fixed draws make every run test the same inputs."""
import random

import numpy as np
import pytest
import torch


@pytest.fixture(autouse=True)
def _fixed_seed():
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
