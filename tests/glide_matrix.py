"""The ledger of glide_kernel's instantiations (csrc/smmc_kernels.hip: GlideFamily::get): template arguments
<kMode, kExactDiv, kDense, K, kVarying> -- three rungs of the mode ladder x two divides x K = 2, 3, 4 x a constant or a
per-period schedule, 36 rows.  One asset has no row: such a request is smmc_engine_simulate_portfolio_cashflow's launch.
tests/test_glide_cpu.py asserts that ROWS names exactly the instantiations the kernels compile to (names only, read with
tools/isa_table.instantiations) and that tests/glide_reference.py's CASES hold one case per row; tests/test_glide_gpu.py
runs them."""
KERNEL = "glide_kernel"
SIGNATURE = "ibbib"  # the template parameters as the Itanium ABI spells their types (i: int, b: bool)
MODE_TABLE, MODE_GAUSSIAN = 0, 1
ASSETS = (2, 3, 4)
# (kMode, kDense) of the ladder's rungs: Gaussian, dense table (eight draws per Philox block), four-draw table
RUNGS = ((MODE_GAUSSIAN, False), (MODE_TABLE, True), (MODE_TABLE, False))
ROWS = [(kmode, exact, dense, K, varying) for kmode, dense in RUNGS for exact in (False, True) for K in ASSETS for varying in (False, True)]


def mangled(args):
    """The template-argument list of an instantiation as it appears in the kernel's symbol: I Li1E Lb0E ... E."""
    return "I" + "".join(f"L{t}{int(v)}E" for t, v in zip(SIGNATURE, args)) + "E"
