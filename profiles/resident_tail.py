"""What heightpitch_resident_bench.py and hpeval_resident_bench.py share: the tail of a resident call alone, by device events."""
from mvoscalerecovery_amd import stream


def tail_us(call, n, repeats, carried):
    """The ``n`` frames of ``call`` (an hp_resident.ResidentCall nothing of which has run) as ONE resident chunk through the driver's
    ``start``, then ``repeats`` launches of its tail alone, nothing downloaded, between two events -> (us per launch, ``carried(st)``:
    the chunk's carried frames)."""
    ctx = call.ctx
    call.chain.append(ctx.to_device(call.carry0))
    st = call.start(0, n, 0)
    try:
        count = carried(st)
        assert int(st["small"]["error"].download()[0]) == -1
        ev = ctx.event(), ctx.event()
        ctx.record(ev[0])
        for _ in range(repeats):
            call.tail(st, n, download=False)
        ctx.record(ev[1])
        ctx.sync()
        us = 1e3 * ctx.elapsed_ms(*ev) / repeats
        for e in ev:
            ctx.lib.mvosr_event_destroy(ctx.handle, e)
    finally:
        stream.free_blocks(st)
        for buf in call.chain:
            buf.free()
    return us, count
