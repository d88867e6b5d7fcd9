"""In-kernel timeline of pn_fwd_screen_kernel (A/B build: python tools/build_ab.py psprof pointnet_enc.hip -DPS_PROFILE
prints the library's path; PARTMANIP_HIP_LIB=<that path> python tools/ps_profile.py).  Ten cycle-counter stamps per wave and tile for work-groups
0-3 (one cloud each, tiles 0-15): loop top | after layer 1 | after the layer-2 MFMA loop | after barrier 3 | after the layer-2
epilogue (tanh, fp16 plane, next tile's points) | after barrier 4 | after the screen MFMA loop | after select / scan | after the
survivor finish | after the h2_save copy.  A segment that ends behind a barrier holds the wait for the slowest wave; the MFMA
segments end when the last MFMA is ISSUED, so their tail lands in the next segment.  The stamps themselves cost a few cycles
each: read the shares.  PN_SAVE_H2=0 profiles the inference forward (no copy)."""
import ctypes, os, sys, torch
sys.path.insert(0, '.')
from partmanip_amd.algo_utils import ActorCritic
from partmanip_amd._lib import lib
DEV = 'cuda:0'
net = dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=False, precision="f32",
           save_h2=os.environ.get("PN_SAVE_H2", "1") == "1")
torch.manual_seed(0)
ac = ActorCritic(3072, 10, dict(action_std=0.5, action_activate="tanh", clipAction=1.0, network=net)).to(DEV)
ac.flat()
B = 2048
x = (torch.rand(B, 1024, 3, device=DEV) * 2 - 1).reshape(B, -1).contiguous()
for _ in range(3):
    ac.actor.hip_forward(x)
torch.cuda.synchronize()
NWG, NTL, NWV, NST = 4, 16, 8, 10
buf = torch.zeros(NWG * NTL * NWV * 16, dtype=torch.int64)
lib.pm_debug_ps_prof_read.argtypes = [ctypes.c_void_p]
assert lib.pm_debug_ps_prof_read(buf.data_ptr()) == 0
t = buf.view(NWG, NTL, NWV, 16)[..., :NST].double()          # [wg][tile][wave][stamp]
names = ["barrier 1 + layer 1", "barrier 2 + layer-2 MFMA", "barrier 3 wait", "layer-2 epilogue", "barrier 4 wait", "screen MFMA loop",
         "select / scan", "survivor finish", "h2_save copy", "to the next loop top"]
tot = torch.zeros(len(names))
for wg in range(NWG):
    s = t[wg, 1:NTL - 1]                     # steady-state tiles (tile 0 holds the cloud's long finish: printed below)
    nxt = t[wg, 2:NTL, :, 0]                 # the next tile's loop top
    d = torch.stack([s[..., i + 1] - s[..., i] for i in range(NST - 1)] + [nxt - s[..., NST - 1]], -1)      # [tile][wave][NST]
    period = (nxt - s[..., 0]).mean()
    print(f"wg {wg}: tile period {period:.0f} cycles (tiles 1-14)")
    for i, n in enumerate(names):
        print(f"   {n:26s} mean {d[..., i].mean():7.0f} ({100 * d[..., i].mean() / period:4.1f} %)   min-wave {d[..., i].mean(0).min():7.0f}"
              f"   max-wave {d[..., i].mean(0).max():7.0f}")
    tot += d.mean((0, 1)).float()
    d0 = torch.stack([t[wg, 0, :, i + 1] - t[wg, 0, :, i] for i in range(NST - 1)], -1)
    print(f"   tile 0: select / scan {d0[:, 6].mean():.0f}, survivor finish mean {d0[:, 7].mean():.0f} max-wave {d0[:, 7].max():.0f}; "
          f"tile 0 loop top -> tile 1 loop top {(t[wg, 1, :, 0] - t[wg, 0, :, 0]).mean():.0f}")
print("all four work-groups, mean cycles per tile and wave: " + ", ".join(f"{n} {v:.0f}" for n, v in zip(names, (tot / NWG).tolist())))
