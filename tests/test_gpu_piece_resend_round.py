"""piecerequest.ReserveRound and ResendRound in turn driving simulated torrents to completion: 1,000,
65 and 1 piece, 5 peers each.  One peer never delivers, and every piece it holds is also held by a
peer that does; the mock clock is stepped past the request timeout every few rounds, so that the
requests the dead peer sits on expire and are resent.  The torrents complete; every resend target
held the piece; no expired request went back to its own peer; outside endgame no piece ever has two
live requests; and the GPU placement's drive (krk_piece_request_round_dev,
krk_piece_resend_round_dev) equals the host placement's resend for resend and pick for pick.  The
host placement runs without a GPU; the GPU placement is marked gpu."""
import numpy as np
import pytest

from kraken_amd import piecerequest as PR

SIZES = (1000, 65, 1)
N_PEERS = 5
LIMIT = 3
TIMEOUT = 5
DEAD = "peer-1"
EVERY = 3  # rounds between two steps of the clock


def dispatchers(policy, disable_endgame):
    ds = []
    for t, n in enumerate(SIZES):
        rng = np.random.default_rng([20261021, n])
        have_it = rng.random((N_PEERS, n)) < 0.4
        live = np.array([p for p in range(N_PEERS) if f"peer-{p}" != DEAD])
        have_it[live[rng.integers(0, live.size, size=n)], np.arange(n)] = True  # a live peer holds every piece
        d = PR.Dispatcher(n, PR.NewManager(PR.MockClock(), TIMEOUT, policy, LIMIT, seed=t + 1), disable_endgame=disable_endgame)
        for p in range(N_PEERS):
            d.AddPeer(f"peer-{p}", have_it[p])
        ds.append(d)
    return ds


def live_requests(d, i):
    return [r for r in d.manager.requests.get(i, ()) if d.manager._live(r)]


def drive(placement, policy, disable_endgame):
    """Every round's outcome until every torrent is complete: ("reserve", [{peerID: [pieces]} a
    torrent]) and ("resend", [[(piece, from peer, status, target)] a torrent]) in turn."""
    ds = dispatchers(policy, disable_endgame)
    rounds, resent = [], 0
    for k in range(2000):
        if all(d.have.all() for d in ds):
            break
        got = PR.ReserveRound(ds, placement=placement)
        rounds.append(("reserve", got))
        for d, g in zip(ds, got):
            for peerID, pieces in g.items():
                for i in pieces if peerID != DEAD else ():  # the pieces of the live peers arrive
                    d.have[i] = True
                    d.manager.Clear(i)
        if k % EVERY == EVERY - 1:
            for d in ds:
                d.manager.clock.Add(TIMEOUT + 1)
        endgame = [d.endgame() for d in ds]
        had = [d.have.copy() for d in ds]
        again = PR.ResendRound(ds, placement=placement)
        rounds.append(("resend", [[(r.Piece, r.PeerID, r.Status, t) for r, t in g] for g in again]))
        for d, g, eg, h in zip(ds, again, endgame, had):
            for r, target in g:
                if target is None:
                    continue
                resent += 1
                assert d.peers[target][r.Piece] and not h[r.Piece], (r, target)  # the target held the piece
                assert not (r.Status == PR.StatusExpired and target == r.PeerID), (r, target)
            for i in {r.Piece for r, _ in g}:
                assert eg or len(live_requests(d, i)) <= 1, (i, live_requests(d, i))
            for r, target in g:  # a resent piece arrives unless the dead peer got it
                if target is not None and target != DEAD and not d.have[r.Piece]:
                    d.have[r.Piece] = True
                    d.manager.Clear(r.Piece)
    assert all(d.have.all() for d in ds), [int(d.have.sum()) for d in ds]
    assert all(not d.manager.requests for d in ds)
    assert resent > 0  # the dead peer's requests went somewhere
    return rounds


@pytest.mark.parametrize("policy", [PR.RarestFirstPolicy, PR.DefaultPolicy])
@pytest.mark.parametrize("disable_endgame", [True, False])
def test_host_rounds_complete_the_torrents(policy, disable_endgame):
    rounds = drive("host", policy, disable_endgame)
    assert any(t == DEAD for kind, got in rounds if kind == "reserve" for g in got for t, pieces in g.items() if pieces)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [PR.RarestFirstPolicy, PR.DefaultPolicy])
@pytest.mark.parametrize("disable_endgame", [True, False])
def test_gpu_drive_equals_the_host_drive(gpu, policy, disable_endgame):
    assert drive("gpu", policy, disable_endgame) == drive("host", policy, disable_endgame)
