// compressed_keygen.cpp -- test program (tests/test_compressed_keys_cpu.py): generates a key set through the shim's TFHE API
// (new_random_gate_bootstrapping_secret_keyset) with the parameters of a named set at a reduced LWE dimension, and writes
// secret.key and cloud.key through the exporters, the way client/gen_secure_keyset.cpp does. Under REDSEC_KEY_FORMAT=compressed
// the cloud key is RSZ1. Never touches the GPU.
#include <cstdlib>
#include <cstring>

#include <tfhe/tfhe.h>
#include <tfhe/tfhe_io.h>

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s n N l Bgbit t basebit ks_stdev bk_stdev secret.key cloud.key\n", argv[0]);
    return 2;
  }
  const int n = atoi(argv[1]), N = atoi(argv[2]), l = atoi(argv[3]), bgbit = atoi(argv[4]), t = atoi(argv[5]), basebit = atoi(argv[6]);
  const double ks_stdev = atof(argv[7]), bk_stdev = atof(argv[8]);
  LweParams* lp = new_LweParams(n, ks_stdev, 0.012467);
  TLweParams* tp = new_TLweParams(N, 1, bk_stdev, 0.012467);
  TGswParams* gp = new_TGswParams(l, bgbit, tp);
  TFheGateBootstrappingParameterSet* p = new TFheGateBootstrappingParameterSet(t, basebit, lp, gp);
  uint32_t seed[] = {314, 1592, 657};
  tfhe_random_generator_setSeed(seed, 3);
  TFheGateBootstrappingSecretKeySet* key = new_random_gate_bootstrapping_secret_keyset(p);
  FILE* f = fopen(argv[9], "wb");
  if (!f) return 3;
  export_tfheGateBootstrappingSecretKeySet_toFile(f, key);
  fclose(f);
  f = fopen(argv[10], "wb");
  if (!f) return 3;
  export_tfheGateBootstrappingCloudKeySet_toFile(f, &key->cloud);
  fclose(f);
  delete_gate_bootstrapping_secret_keyset(key);
  return 0;
}
