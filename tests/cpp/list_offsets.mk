# host test of the list loader's offset check (csrc/list_offsets.h), under the address and undefined-behaviour sanitizers:
#   make -C tests/cpp -f list_offsets.mk
ROOT := ../..
CXX  ?= g++
all: test_list_offsets
test_list_offsets: test_list_offsets.cpp $(ROOT)/vector_line_quantization_amd/csrc/list_offsets.h $(ROOT)/include/vlq_ivfpq.h
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -I$(ROOT)/vector_line_quantization_amd/csrc $< -o $@
clean:
	rm -f test_list_offsets
.PHONY: all clean
