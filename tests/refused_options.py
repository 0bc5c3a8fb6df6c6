"""What both builds of the library refuse since the experiments that lost were removed (include/lam_hip_tuning.md, "Removed"):
shared by tests/test_gpu_parity.py::test_tuning_build_variants (product library) and tests/tuning_cases.py `refusals` (tuning build)."""

KEPT_VARIANTS = (-1, 0, 10, 13, 17)           # the dtypes' production shapes + the 4-rows-per-8-waves option
MFMA_VARIANTS = (20, 21)                      # tuning build, bf16 storage only
REMOVED_VARIANTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 15, 16, 18, 19, 22, 23, 24, 25, 26, 27)
NEVER_VARIANTS = (28, 1000)                   # never existed
REMOVED_OPTIONS = ("persistent", "persist_chunk", "host_threads", "exchange_hub")
REMOVED_READ_ONLY = ("persistent_effective", "persistent_workers")


def refused(lam, call, *args):
    """The call fails with LAM_HIP_EINVAL (-1)."""
    try:
        call(*args)
    except lam.LamHipError as e:
        return e.code == -1
    return False


def check_removed(lam, s):
    """Every removed GEMV number and option name is refused by solver `s`, for value 0 as for value 1, and cannot be read."""
    for v in REMOVED_VARIANTS + NEVER_VARIANTS:
        assert refused(lam, s.set_option, "gemv_variant", v), v
    assert s.get_option("gemv_variant") == -1                      # a refused number leaves the option alone
    for name in REMOVED_OPTIONS:
        for value in (0, 1):
            assert refused(lam, s.set_option, name, value), (name, value)
    for name in REMOVED_OPTIONS + REMOVED_READ_ONLY:
        assert refused(lam, s.get_option, name), name
