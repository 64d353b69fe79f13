"""The convolutional predictor on a tile-sharded cube: two ranks (gloo rendezvous; both use cuda:0 here, one GPU per rank on
a node) hold three tiles each with their data on the device.  The halo cells a rank's tiles need from the other rank's come
through ``parallel.exchange_edge_strips`` -- one all-gather of the edge strips, staged through the host on gloo.  The sharded
prediction must equal the single-process prediction of the resident cube bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import conv_cases

pytestmark = pytest.mark.gpu
N = 12


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _model_and_cube():
    import fv3net_amd.fit as fit

    rng = np.random.default_rng(70)
    spec = conv_cases.make_spec(rng, {"T": 19, "lat": 1}, 32, 3, 3, {"dQ1": 19, "rain": 1}, activation="tanh")
    cube = conv_cases.make_inputs(rng, spec, (2, 6), N, N)  # [time, tile, x, y, z], the same on every rank
    cube["lat"] = cube["lat"].astype(np.float64)
    return fit.HipConvolutionalModel(["T", "lat"], ["dQ1", "rain"], spec), cube


def _dataset(cube, tiles, dev):
    from fv3net_amd.xr_compat import DataArray, Dataset

    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return Dataset({
        "T": DataArray(put(cube["T"][:, tiles]), dims=("time", "tile", "x", "y", "z"), coords={"tile": np.asarray(tiles)}),
        "lat": DataArray(put(cube["lat"][..., 0][:, tiles].transpose(1, 3, 2, 0)), dims=("tile", "y", "x", "time")),
    })


def _worker(rank, size, port, out_dir):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=size)
    torch.cuda.set_device(0)
    from fv3net_amd import parallel

    model, cube = _model_and_cube()
    mine = parallel.tiles_of_rank(size, rank)
    out = model.predict(_dataset(cube, mine, torch.device("cuda:0")))
    assert out["dQ1"].data.is_cuda and out["dQ1"].dims == ("time", "tile", "x", "y", "z")
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), tiles=np.asarray(mine),
             **{name: out[name].data.cpu().numpy() for name in ("dQ1", "rain")})
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_tile_sharded_prediction(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    model, cube = _model_and_cube()
    ref = model.predict(_dataset(cube, list(range(6)), torch.device("cuda:0")))
    for rank in range(2):
        with np.load(tmp_path / f"rank{rank}.npz") as z:
            tiles = z["tiles"].tolist()
            assert tiles == [[0, 1, 2], [3, 4, 5]][rank]
            for name in ("dQ1", "rain"):
                want = ref[name].data.cpu().numpy()[:, tiles]
                assert want.shape[2:4] == (N, N)
                np.testing.assert_array_equal(z[name], want, err_msg=f"{name} rank {rank}")
