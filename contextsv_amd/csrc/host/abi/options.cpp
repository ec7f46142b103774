// options.cpp — the run options' defaults: RunParams' own (run_options.hpp), nothing restated here
#include "run_options.hpp"

extern "C" void csvhost_run_options_init(csvhost_run_options *opt) { run_options_from(RunParams(), *opt); }
