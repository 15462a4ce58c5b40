"""Worker of tests/test_gpu_gnn.py::test_device_tensors_are_not_staged: torch first, then the engine, so that one HIP runtime serves
both and the engine can take views of torch's device memory (include/pgh_gnn.h pgh_mat_wrap)."""
import os
import sys

import torch                      # before anything loads the engine library

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):
    if path not in sys.path:
        sys.path.insert(0, path)


def main():
    import pygrank_amd as pg
    from pygrank_amd import _lib
    from oracle import rmat_np
    import test_gpu_gnn as checks
    assert torch.cuda.is_available(), "torch sees no GPU"
    pg.load_backend("hip")
    assert _lib.runtime_name().startswith("hip:")
    case = checks.Case(pg, rmat_np.rmat_csr(11, 8, seed=5), True, "col")
    widths = [20, 70]
    for b in widths:
        checks.device_tensor_checks(pg, case, b)
    print("device tensors: ok", widths)


if __name__ == "__main__":
    main()
