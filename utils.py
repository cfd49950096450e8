"""Reference-compatible ``utils`` module (``prepare_batch``, ``generate``, ``generate_batch``)."""
from distributed_pytorch_cookbook_amd.utils.batch import generate, generate_batch, prepare_batch  # noqa: F401
