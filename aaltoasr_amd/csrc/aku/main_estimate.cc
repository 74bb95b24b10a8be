// estimate -- model re-estimation with the reference tool's options (aku/estimate.cc:115-155) on the engine: the
// dumps of stats (.gks / .mcs / .phs / .lls) added on the host, the ML update, the pool edits (--delete, --mremove,
// --split) and the writers on the host, MLLT (--mllt MODULE) over resident covariances on the device
// (aasr_run_estimate).
//
//   estimate (-b BASE | -g GK -m MC -p PH) -L LIST -o OUT --ml [-c CFG] [-t] [--mllt MODULE] [--minvar V]
//            [--covsmooth C] [--delete OCC] [--mremove W] [--split (--minocc OCC | --numgauss N) [--maxmixgauss N]
//            [--splitalpha A]] [--no-mixture-update] [--no-write] [-s SUMMARY] [-i level]
//
// Refused before anything is read: --mmi, --mpe and the EBW options (--C1, --C2, --ismooth, --mmi-prior-ismooth,
// --prev-prior, --limit, --silence-d, -D, --write-ebwd), -C and the --hcl-* options (subspace Gaussians),
// --no-silence-update; pools with full-covariance or subspace Gaussians.  The device is opened only for --mllt and for
// writing OUT.cfg.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: estimate [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "Previous base filename for model files")
    ('g', "gk=FILE", "arg", "", "Previous mixture base distributions")
    ('m', "mc=FILE", "arg", "", "Previous mixture coefficients for the states")
    ('p', "ph=FILE", "arg", "", "Previous HMM definitions")
    ('c', "config=FILE", "arg", "", "feature configuration (required for MLLT)")
    ('L', "list=LISTNAME", "arg must", "", "file with one statistics file per line")
    ('C', "coeffs=NAME", "arg", "", "Precomputed precision/subspace Gaussians")
    ('o', "out=BASENAME", "arg must", "", "base filename for output models")
    ('t', "transitions", "", "", "estimate also state transitions")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "mllt=MODULE", "arg", "", "update maximum likelihood linear transform")
    ('\0', "ml", "", "", "maximum likelihood estimation")
    ('\0', "mmi", "", "", "maximum mutual information estimation")
    ('\0', "mpe", "", "", "minimum phone error estimation")
    ('\0', "minvar=FLOAT", "arg", "0.1", "minimum variance (default 0.1)")
    ('\0', "covsmooth", "arg", "0", "covariance smoothing (default 0.0)")
    ('\0', "C1=FLOAT", "arg", "2.0", "constant \"C1\" for EBW updates (default 2.0)")
    ('\0', "C2=FLOAT", "arg", "2.0", "constant \"C2\" for EBW updates (default 2.0)")
    ('\0', "ismooth=FLOAT", "arg", "0.0", "I-smoothing constant")
    ('\0', "mmi-prior-ismooth=FLOAT", "arg", "0.0", "Use MMI prior when I-smoothing MPE model")
    ('\0', "prev-prior", "", "", "Use previous model as prior in I-smoothing")
    ('\0', "limit", "arg", "0.0", "Global KLD limit for parameter change")
    ('\0', "delete=FLOAT", "arg", "0.0", "delete Gaussians with occupancies below the threshold")
    ('\0', "mremove=FLOAT", "arg", "0.0", "remove mixture components below the weight threshold")
    ('\0', "split", "", "", "Enable Gaussian splitting")
    ('\0', "minocc=FLOAT", "arg", "0.0", "Occupancy threshold for Gaussian splitting")
    ('\0', "maxmixgauss=INT", "arg", "0", "maximum number of Gaussians per mixture for splitting")
    ('\0', "numgauss=INT", "arg", "-1", "Target number of Gaussians in the final model")
    ('\0', "splitalpha=FLOAT", "arg", "1.0", "Occupancy smoothing power for splitting")
    ('\0', "no-silence-update", "", "", "Don't update silence state parameters")
    ('\0', "no-mixture-update", "", "", "Do not update mixture coefficients")
    ('\0', "silence-d=FLOAT", "arg", "0", "Set a fixed EBW D for silence Gaussians")
    ('D', "ebwd=FILE", "arg", "", "Read Gaussian specific EBW D values (and limits)")
    ('\0', "write-ebwd=FILE", "arg", "", "Write Gaussian specific D and minimum D values")
    ('\0', "no-write", "", "", "Don't write anything")
    ('s', "savesum=FILE", "arg", "", "save summary information")
    ('\0', "hcl-bfgs-cfg=FILE", "arg", "", "configuration file for HCL biconjugate gradient algorithm")
    ('\0', "hcl-line-cfg=FILE", "arg", "", "configuration file for HCL line search algorithm")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  // what this build does not do, refused before anything is read
  const char *refused[][2] = {{"mmi", "--mmi (discriminative estimation)"},
                              {"mpe", "--mpe (discriminative estimation)"},
                              {"C1", "--C1 (EBW update)"},
                              {"C2", "--C2 (EBW update)"},
                              {"ismooth", "--ismooth (EBW update)"},
                              {"mmi-prior-ismooth", "--mmi-prior-ismooth (EBW update)"},
                              {"prev-prior", "--prev-prior (EBW update)"},
                              {"limit", "--limit (EBW update)"},
                              {"silence-d", "--silence-d (EBW update)"},
                              {"ebwd", "-D (EBW update)"},
                              {"write-ebwd", "--write-ebwd (EBW update)"},
                              {"coeffs", "-C (subspace Gaussians)"},
                              {"hcl-bfgs-cfg", "--hcl-bfgs-cfg (subspace Gaussians)"},
                              {"hcl-line-cfg", "--hcl-line-cfg (subspace Gaussians)"},
                              {"no-silence-update", "--no-silence-update"}};
  int count = 0;
  for (const char *m : {"ml", "mmi", "mpe"})
    if (config[m].specified) count++;
  if (count != 1) die("Define exactly one of --ml, --mmi and --mpe!");
  for (const auto &r : refused)
    if (config[r[0]].specified) die(std::string("estimate: ") + r[1] + " is not supported; only --ml estimation of diagonal Gaussians is");

  if (config["split"].specified && !(config["minocc"].specified || config["numgauss"].specified)) {
    fprintf(stderr, "Either --minocc or --numgauss is required with --split\n");
    exit(1);
  }
  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  check_pool(gk, "estimate");
  if (config["mllt"].specified && !config["config"].specified) die("Must specify configuration file with MLLT");

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  aasr_estimate_options opt;
  aasr_estimate_default_options(&opt);
  const std::string base = config["base"].specified ? config["base"].get_str() : gk, cfg = config["config"].get_str(),
                    list = config["list"].get_str(), out = config["out"].get_str(), mllt = config["mllt"].get_str(),
                    savesum = config["savesum"].get_str();
  opt.gk = gk.c_str();
  opt.mc = mc.c_str();
  opt.ph = ph.c_str();
  opt.base_name = base.c_str();
  opt.config = config["config"].specified ? cfg.c_str() : nullptr;
  opt.list = list.c_str();
  opt.out = out.c_str();
  opt.mllt = config["mllt"].specified ? mllt.c_str() : nullptr;
  opt.savesum = config["savesum"].specified ? savesum.c_str() : nullptr;
  opt.transitions = config["transitions"].specified;
  opt.info = config["info"].get_int();
  opt.minvar = config["minvar"].get_double();
  opt.covsmooth = config["covsmooth"].get_double();
  opt.delete_set = config["delete"].specified;
  opt.delete_minocc = config["delete"].get_double();
  opt.mremove_set = config["mremove"].specified;
  opt.mremove = config["mremove"].get_double();
  opt.split = config["split"].specified;
  opt.minocc_set = config["minocc"].specified;
  opt.minocc = config["minocc"].get_double();
  opt.maxmixgauss = config["maxmixgauss"].get_int();
  opt.numgauss_set = config["numgauss"].specified;
  opt.numgauss = config["numgauss"].get_int();
  opt.splitalpha = config["splitalpha"].get_double();
  opt.no_mixture_update = config["no-mixture-update"].specified;
  opt.no_write = config["no-write"].specified;
  if (aasr_run_estimate(&opt) != AASR_OK) die(aasr_last_error());
  if (opt.info > 0) {
    printf("Read the statistics in %.3f s\n", opt.seconds_read);
    if (opt.mllt) printf("MLLT in %.3f s\n", opt.seconds_mllt);
    if (opt.delete_set) printf("Deleted %d Gaussians\n", opt.n_deleted);
    if (opt.mremove_set) printf("Removed %d Gaussians without a mixture\n", opt.n_removed);
    if (opt.split) printf("Split %d Gaussians\n", opt.n_splits);
  }
  return 0;
}
