"""CPU: the frame kernel's tile-order switch (ngp_render_set_tile_order) is declared, exported, on by default, returns the previous setting, and its
cost-ordered hand-out leaves the workspace size -- part of the C ABI -- as it was: header + 48 KiB + two u32 per 64 rays."""


def test_tile_order_switch_round_trip():
    import ngp_hip
    L = ngp_hip.lib()
    assert "ngp_render_set_tile_order" in ngp_hip.EXPORTS
    assert L.ngp_render_set_tile_order(0) == 1                   # default on
    try:
        assert L.ngp_render_set_tile_order(1) == 0
        assert L.ngp_render_set_tile_order(7) == 1               # any non-zero value means on
    finally:
        L.ngp_render_set_tile_order(1)


def test_workspace_holds_a_permutation_and_a_cost_per_tile():
    import ngp_hip
    L = ngp_hip.lib()
    for n in (64, 640_000, 40_000, 8 * 640_000):
        assert L.ngp_render_frame_workspace(n) == 256 + 48 * 1024 + 8 * ((n + 63) // 64)
