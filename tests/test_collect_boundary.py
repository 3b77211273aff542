"""CPU-side checks of the sample-collection stage's boundary: the header declares its three entries,
the ctypes table binds them and the library exports them; argument errors are reported through
cacto_last_error without a GPU; the ABI version is unchanged; cacto_amd.main's parser maps the
reference's options and the three of this package."""
import pytest

from cacto_amd import _lib as L

ENTRIES = ("cacto_env_rl_episodes", "cacto_collect_plan", "cacto_episode_returns")


def test_header_declares_the_entries_and_the_library_exports_them():
    names = L.header_exports()
    lib = L.lib()
    for n in ENTRIES:
        assert n in names and n in L._SIGS and hasattr(lib.dll, n)
    assert lib.dll.cacto_abi_version() == 1


def test_argument_errors_without_a_gpu():
    lib = L.lib()
    one = 8          # a non-null address that is never dereferenced: every call below is refused first
    with pytest.raises(RuntimeError, match="cacto_env_rl_episodes: bad arguments"):
        lib.call("cacto_env_rl_episodes", None, None, None, 1, None, 1, 2, None, None, None, None)
    for ldU, n_ep, ldS in ((0, 1, 2), (1, 0, 2), (1, 1, 0), (1, -3, 2)):
        with pytest.raises(RuntimeError, match="cacto_env_rl_episodes: bad arguments"):
            lib.call("cacto_env_rl_episodes", one, one, one, ldU, one, n_ep, ldS, None, None, None, None)
    with pytest.raises(RuntimeError, match="cacto_collect_plan: bad arguments"):
        lib.call("cacto_collect_plan", None, None, None, 0, 1, None, None, None, None)
    for nsteps, n_ep, kept, off, counts in ((None, 1, one, one, one), (one, 0, one, one, one), (one, -1, one, one, one),
                                            (one, 1, None, one, one), (one, 1, one, None, one),
                                            (one, 1, one, one, None)):
        with pytest.raises(RuntimeError, match="cacto_collect_plan: bad arguments"):
            lib.call("cacto_collect_plan", nsteps, None, None, 1, n_ep, kept, off, counts, None)
    with pytest.raises(RuntimeError, match="cacto_episode_returns: bad arguments"):
        lib.call("cacto_episode_returns", None, 1, None, 1, 0, None, None)
    for R, ldR, kept, n_ep, ret in ((one, 0, one, 1, one), (one, 1, one, 0, one), (one, 1, None, 1, one),
                                    (one, 1, one, 1, None), (None, 1, one, 1, one)):
        with pytest.raises(RuntimeError, match="cacto_episode_returns: bad arguments"):
            lib.call("cacto_episode_returns", R, ldR, kept, n_ep, 1, ret, None)


def test_main_parser_maps_the_options():
    from cacto_amd import main as M
    a = M.parse_args([])
    assert a == dict(test_n=0, seed=0, system_id="single_integrator", recover_training_flag=False, w_S=0,
                     nb_loops=None, to_path="default", accept_maxiter=False)
    a = M.parse_args(["--system-id", "double_integrator", "--seed", "3", "--test-n", "2", "--w-S", "1e-2",
                      "--recover-training-flag", "--nb-loops", "1", "--to-path", "wave", "--accept-maxiter"])
    assert a == dict(test_n=2, seed=3, system_id="double_integrator", recover_training_flag=True, w_S=1e-2,
                     nb_loops=1, to_path="wave", accept_maxiter=True)
    system_id, kw = M.train_kwargs(a)
    assert system_id == "double_integrator"
    assert kw == dict(seed=3, N_try=2, w_S=1e-2, to_cfg=dict(path="wave"), accept_maxiter=True, n_loops=1,
                      recover=True)
    with pytest.raises(SystemExit):
        M.parse_args(["--system-id", "pendulum"])
    with pytest.raises(SystemExit):
        M.parse_args(["--to-path", "fast"])
