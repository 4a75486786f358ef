// seeded_export.cpp -- test program (tests/test_seeded_ciphertexts_cpu.py): encrypts bits through the shim's TFHE API
// (bootsSymEncrypt) under a key set of a small LWE dimension, exports them with export_gate_bootstrapping_ciphertext_toFile and
// reads them back with import_gate_bootstrapping_ciphertext_fromFile. Under REDSEC_CT_FORMAT=seeded the file is RSC1.
//   mode roundtrip   export 5 samples, read them back twice (two opens of the file), print the decrypted bits and mask equality
//   mode modified    lweAddTo on sample 1 before its export (the shim must refuse it under REDSEC_CT_FORMAT=seeded)
//   mode gap         export samples 0 and 2 (the shim must refuse the gap under REDSEC_CT_FORMAT=seeded)
// Never touches the GPU.
#include <cstdlib>
#include <cstring>

#include <tfhe/tfhe.h>
#include <tfhe/tfhe_io.h>

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s roundtrip|modified|gap file\n", argv[0]);
    return 2;
  }
  const char* mode = argv[1];
  LweParams* lp = new_LweParams(40, 0x1p-25, 0.012467);
  TLweParams* tp = new_TLweParams(1024, 1, 0x1p-30, 0.012467);
  TGswParams* gp = new_TGswParams(10, 3, tp);
  TFheGateBootstrappingParameterSet* p = new TFheGateBootstrappingParameterSet(9, 3, lp, gp);
  TFheGateBootstrappingSecretKeySet* key = new_random_gate_bootstrapping_secret_keyset(p);
  const int bits[5] = {1, 0, 0, 1, 1};
  LweSample* ct = new_gate_bootstrapping_ciphertext_array(5, p);
  for (int i = 0; i < 5; ++i) bootsSymEncrypt(&ct[i], bits[i], key);
  FILE* f = fopen(argv[2], "wb");
  if (!strcmp(mode, "modified")) lweAddTo(&ct[1], &ct[0], lp);
  for (int i = 0; i < 5; ++i)
    if (strcmp(mode, "gap") || i != 1) export_gate_bootstrapping_ciphertext_toFile(f, &ct[i], p);
  fclose(f);
  LweSample* back = new_gate_bootstrapping_ciphertext_array(5, p);
  for (int pass = 0; pass < 2; ++pass) {
    f = fopen(argv[2], "rb");
    int same = 1;
    for (int i = 0; i < 5; ++i) {
      import_gate_bootstrapping_ciphertext_fromFile(f, &back[i], p);
      printf("%d", bootsSymDecrypt(&back[i], key));
      same &= back[i].b == ct[i].b && !memcmp(back[i].a, ct[i].a, sizeof(Torus32) * 40);
    }
    printf(" same=%d\n", same);
    fclose(f);
  }
  delete_gate_bootstrapping_ciphertext_array(5, back);
  delete_gate_bootstrapping_ciphertext_array(5, ct);
  delete_gate_bootstrapping_secret_keyset(key);
  return 0;
}
