"""Survivor / fallback counters of the screened PointNet forward (csrc/pointnet_enc_screen.h) on the clouds real runs feed:
the bench's uniform cubes, posed mesh surface clouds (FeederEnv with a PCfromMesh source over synthetic box parts) and the feeder's uniform cubes at 4096
points per cloud (the point count of the DAgger bench's student; NOT a batch taken from the DAgger path).  Default-initialised weights; one JSON line per case.  GPU box only."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partmanip_amd.algo_utils import ActorCritic  # noqa: E402
from partmanip_amd.feeder import FeederEnv  # noqa: E402
from partmanip_amd.mesh2pc import PCfromMesh  # noqa: E402
from tools.time_mesh_pc import synthetic_parts  # noqa: E402

DEV = "cuda:0"


def case(name, B, P, pc_source=None, sub_mean=False):
    net = dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=sub_mean, point_num=P)
    torch.manual_seed(0)
    ac = ActorCritic(3 * P, 10, dict(action_std=0.5, action_activate="tanh", clipAction=1.0, network=net)).to(DEV)
    ac.flat()
    env = FeederEnv(B, {"obs": 3 * P}, 10, DEV, seed=1234, point_num=P, pc_source=pc_source)
    x = env.reset()["obs"]
    ac.actor.screen_counters = torch.zeros(3, dtype=torch.int64, device=DEV)
    ac.actor.hip_forward(x, save_h2=False)
    s, fb, hit = ac.actor.screen_counters.tolist()
    tiles = P // 64
    print(json.dumps(dict(case=name, clouds=B, points=P, sub_mean=sub_mean, survivors_per_cloud_channel=s / (B * 512),
                          fallback_wave_tiles=fb, wave_tiles=B * tiles * 8, tile_channel_pairs_hit=hit / (B * tiles * 512))), flush=True)


if __name__ == "__main__":
    case("bench uniform cubes", 2048, 1024)
    for sub in (False, True):
        case("posed mesh clouds (12 box parts)", 2048, 1024, PCfromMesh(2048, DEV, num_points=1024, part_pcs=synthetic_parts(12, 1024)), sub)
    case("uniform cubes, 4096 points per cloud", 512, 4096)
