#!/usr/bin/env python3
"""What ordering a pt launch's work items by pixel cost can buy, from a cost map alone (host only, no GPU).

    python tools/cost_order_model.py COST.npy [--price-with OTHER.npy] [--width 1920 --height 1080 --tile 32 --slots 1024] [--json OUT.json]

COST.npy: uint32[H * W] (or [H, W]), closest-hit rays per pixel over one launch -- what a session records (PtParams.item_cost), as a map over the
pixels (PtSession.cost_order(n)["cost"], the test hook akr_probe_pt_cost_order). A lane's time in k_pt_pass is taken to be proportional to that
count: a lane advances one path vertex per iteration of the wave's loop, and every iteration costs the wave one pair walk whatever
its lanes do.

Two dealings of pixels to lanes are compared: by position (dpath.h item_to_pixel: tiles row by row, 8 x 8 squares inside a tile) and by
descending cost (ties by ascending pixel: csrc/cost_order_kernels.hip). For each:

  wave      mean over waves of sum(lane cost) / (64 x max lane cost)        -- lanes that wait for the wave's dearest pixel
            (and the same weighted by the wave's time, sum over waves of sum(lane cost) / sum over waves of 64 x max: the share of
            lane-iterations that do work)
  group     mean over workgroups of sum(wave time) / (4 x max wave time)    -- wave slots and LDS held until the group's dearest wave ends
            (and the same weighted by the group's time)
  tail      greedy makespan of the workgroups in dispatch order on `slots` workgroup slots / (sum of group times / slots)
            -- the launch ends on whichever groups come last

A wave's time is its dearest lane's cost, a workgroup's its dearest wave's.
"""
import argparse
import heapq
import json

import numpy as np

INVALID = 0xFFFFFFFF


def positional_items(width, height, tile):
    """item -> pixel as dpath.h item_to_pixel deals them on one rank; INVALID = out of frame."""
    tiles_x, tiles_y = -(-width // tile), -(-height // tile)
    item = np.arange(tiles_x * tiles_y * tile * tile, dtype=np.int64)
    t, within = item // (tile * tile), item % (tile * tile)
    ty, tx = t // tiles_x, t % tiles_x
    block, lane = within >> 6, within & 63
    bpr = tile >> 3
    by, bx = block // bpr, block % bpr
    px, py = tx * tile + bx * 8 + (lane & 7), ty * tile + by * 8 + (lane >> 3)
    ok = (px < width) & (py < height)
    return np.where(ok, px + py * width, INVALID).astype(np.int64)


def sorted_items(cost, n_items):
    """item -> pixel of the cost order: descending cost, ties by ascending pixel, INVALID padding to the positional item count's multiple of 256."""
    order = np.lexsort((np.arange(cost.size), -cost.astype(np.int64)))
    out = np.full((n_items + 255) // 256 * 256, INVALID, dtype=np.int64)
    out[: cost.size] = order
    return out


def price(items, cost, slots):
    n = (items.size + 255) // 256 * 256
    it = np.full(n, INVALID, dtype=np.int64)
    it[: items.size] = items
    c = np.where(it != INVALID, cost[np.minimum(it, cost.size - 1)], 0).astype(np.float64)
    lanes = c.reshape(-1, 64)
    wave_t, wave_sum = lanes.max(axis=1), lanes.sum(axis=1)
    live = wave_t > 0
    groups = wave_t.reshape(-1, 4)
    group_t, group_sum = groups.max(axis=1), groups.sum(axis=1)
    glive = group_t > 0
    # list scheduling in dispatch order: the next workgroup goes to the slot that frees first
    heap = [0.0] * slots
    for t in group_t[glive]:
        heapq.heappush(heap, heapq.heappop(heap) + t)
    makespan, ideal = max(heap), group_t.sum() / slots
    return {
        "waves": int(live.sum()), "workgroups": int(glive.sum()),
        "wave_mean": float(np.mean(wave_sum[live] / (64.0 * wave_t[live]))),
        "wave_time_weighted": float(wave_sum.sum() / (64.0 * wave_t.sum())),
        "group_mean": float(np.mean(group_sum[glive] / (4.0 * group_t[glive]))),
        "group_time_weighted": float(group_sum.sum() / (4.0 * group_t.sum())),
        "rounds": float(ideal / np.mean(group_t[glive])) if glive.any() else 0.0,
        "tail_makespan_over_ideal": float(makespan / ideal),
        # the launch's modelled time, in wave iterations of the dearest-lane kind: makespan of the groups
        "makespan": float(makespan),
    }


def summary(cost):
    q = np.percentile(cost, [0, 1, 25, 50, 75, 99, 100])
    return {"pixels": int(cost.size), "sum": int(cost.astype(np.uint64).sum()), "mean": float(cost.mean()), "std": float(cost.std()),
            "min_p1_p25_p50_p75_p99_max": [float(x) for x in q]}


def model(cost, width, height, tile=32, slots=1024, price_with=None):
    """price_with: the cost map of ANOTHER launch of the same frame (another seed): the order is made from `cost` and both dealings are
    priced on price_with -- what a session gets, whose later launches are not the one it sorted by. None: priced on `cost` itself, which
    flatters the order by the sampling noise of a pixel's cost."""
    cost = np.asarray(cost).reshape(-1).astype(np.uint32)
    assert cost.size == width * height, (cost.size, width, height)
    paid = cost if price_with is None else np.asarray(price_with).reshape(-1).astype(np.uint32)
    assert paid.size == cost.size
    pos = positional_items(width, height, tile)
    a, b = price(pos, paid, slots), price(sorted_items(cost, pos.size), paid, slots)
    return {"cost_map": summary(cost), "priced_on": "the same launch" if price_with is None else "another launch", "by_position": a, "by_cost": b,
            "predicted_speedup": a["makespan"] / b["makespan"], "slots": slots, "tile": tile}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cost")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tile", type=int, default=32)
    ap.add_argument("--slots", type=int, default=1024, help="workgroups resident at once: 256 CUs x 4 (k_pt_pass: 4 waves per SIMD, 4-wave workgroups)")
    ap.add_argument("--price-with", default=None, metavar="OTHER.npy", help="price both dealings on this launch's cost map (the order still comes from COST.npy)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = model(np.load(a.cost), a.width, a.height, a.tile, a.slots, np.load(a.price_with) if a.price_with else None)
    print(json.dumps(out, indent=1))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
