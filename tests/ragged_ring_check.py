"""The asynchronous-ring check the three ragged GPU test files share: more SVHIP_ASYNC ragged calls in flight on one handle than it has
pinned table slots (four), so the ring wraps and a slot is taken again while calls are still queued."""
import numpy as np
import torch


def check_async_ring(e, wave_packs):
    """wave_packs: six lists of two or three 1-D waveforms.  Every pack is embedded synchronously, then all six with async_=True into
    their own CUDA outputs, the host offsets / lengths of each call zeroed as soon as it returns (the library has copied them by then);
    after Engine.synchronize() every result is its synchronous twin bit for bit (the ragged forward is batch invariant and both runs
    take the same kernels).  A slot handed out while its copy is still in flight shows up as a wrong embedding."""
    assert len(wave_packs) == 6 and all(2 <= len(p) <= 3 for p in wave_packs)
    packs = []
    for wavs in wave_packs:
        lens = np.array([len(w) for w in wavs], dtype=np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        packs.append((torch.from_numpy(np.concatenate(wavs)).cuda(), offs, lens))
    sync = [e.embed_wave_ragged(p, offsets=o, lengths=l).cpu().numpy() for p, o, l in packs]
    assert all(np.isfinite(s).all() for s in sync)
    assert any(not np.array_equal(sync[0][0], s[0]) for s in sync[1:])          # (different packs: a stale table would show)
    torch.cuda.synchronize()
    outs = [torch.full((len(l), e.embed_dim), float("nan"), dtype=torch.float32, device="cuda") for _, _, l in packs]
    torch.cuda.synchronize()
    for (p, o, l), out in zip(packs, outs):
        o, l = o.copy(), l.copy()
        # (int64 / int32 C-contiguous arrays pass through Engine._pack uncopied: the library reads these very arrays, so the zeroing
        # below tests ITS copy.  Whether a slot is still in flight when the ring wraps depends on how far the GPU lags the host;
        # with a lag of fewer than four calls the test still checks the order and the tables of six queued calls.)
        assert np.ascontiguousarray(o, dtype=np.int64) is o and np.ascontiguousarray(l, dtype=np.int32) is l
        ret = e.embed_wave_ragged(p, offsets=o, lengths=l, out=out, async_=True, ordered=True)
        assert ret is out
        o[:] = 0
        l[:] = 0
    e.synchronize()
    for k, (out, want) in enumerate(zip(outs, sync)):
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (k, float(np.abs(got - want).max()))
